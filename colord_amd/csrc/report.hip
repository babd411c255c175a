// report.hip — the content report of a chunk on the device (report.hpp): cl_report_bases over the 2-bit arena,
// cl_report_quals over the input quality bytes; their host counterparts; the pipeline's hook (report_chunk).
//
// k_report_bases has the shape of k_digest_bases: one wave per read, four reads per 256-thread block, the lanes striding over the
// read's arena words; per word five popcounts (rp_block_counts), five wave sums, the block's sums through LDS and ONE 64-bit vector
// atomic add per field into one of RP_SLOTS accumulators chosen by block index.  Lane 0 adds its read to the length histograms.
// k_report_quals is persistent: blocks of four waves stride over quads of reads, a wave walks its read with qual_value_walk
// (qual_walk.hpp — the walk of k_qual_values) and counts every byte with one LDS atomic into the block's 96 x 96 matrix of 32-bit
// cells, which is added to the 64-bit matrix in memory, non-zero cells only, at the block's end and before a cell could wrap.
// Bounds by construction: a read's arena words are [word_off[r], word_off[r + 1]); a quality byte is loaded only at an index inside
// [qoff[r], qoff[r + 1]); `in` and `out` are clamped to 0..95 before they index LDS.
#include "common.hpp"
#include "objects.hpp"
#include "report.hpp"
#include "qual_walk.hpp"
#include <memory>

namespace {
constexpr uint32_t RP_SLOTS = 64;
// the accumulators of k_report_bases: six fields (A, C, G, T, N, bases) x RP_SLOTS, then the length histograms, ~min and max
constexpr uint32_t RB_HIST = 6 * RP_SLOTS, RB_LBASES = RB_HIST + 33, RB_NMIN = RB_LBASES + 33, RB_MAX = RB_NMIN + 1, RB_WORDS = RB_MAX + 1;
// those of k_report_quals: the joint matrix, the mean-quality histogram, the refusal flag
constexpr uint32_t RQ_CELLS = 96 * 96, RQ_MEAN = RQ_CELLS, RQ_ERR = RQ_MEAN + 96, RQ_WORDS = RQ_ERR + 1;
constexpr uint64_t RQ_CELL_MAX = 0xffffffffULL;

__global__ __launch_bounds__(256) void k_report_bases(const uint64_t* __restrict__ packed, const uint32_t* __restrict__ inv, const uint64_t* __restrict__ word_off,
                                                     const uint32_t* __restrict__ lens, uint32_t n_reads, unsigned long long* __restrict__ g)
{
	__shared__ uint64_t s_sum[4][6];
	const uint32_t w = threadIdx.x >> 6, r = blockIdx.x * 4 + w, lane = threadIdx.x & 63;
	uint64_t c[6] = { 0, 0, 0, 0, 0, 0 };
	if (r < n_reads)                                                            // (wave-uniform)
	{
		const uint64_t wb = word_off[r], words = word_off[r + 1] - wb, len = lens[r];
		uint64_t nb = (len + 31) / 32;                                          // blocks that hold bases (k_digest_bases)
		if (nb > words) nb = words;                                             // (never: an arena read has len / 32 + 1 words)
		for (uint64_t b = lane; b < nb; b += 64)
		{
			uint64_t P = packed[wb + b]; uint32_t I = inv[wb + b];
			dg_block(P, I, len - 32 * b);
			uint32_t k[5];
			rp_block_counts(P, I, len - 32 * b, k);
#pragma unroll
			for (uint32_t t = 0; t < 5; ++t) c[t] += k[t];
		}
#pragma unroll
		for (uint32_t t = 0; t < 5; ++t) c[t] = wave_sum64(c[t]);
		c[5] = len;
		if (lane == 0)
		{
			const uint32_t bin = rp_len_bin(len);
			atomicAdd(g + RB_HIST + bin, 1ULL); atomicAdd(g + RB_LBASES + bin, (unsigned long long)len);
			atomicMax(g + RB_NMIN, ~(unsigned long long)len); atomicMax(g + RB_MAX, (unsigned long long)len);
		}
	}
	if (lane == 0)
#pragma unroll
		for (uint32_t t = 0; t < 6; ++t) s_sum[w][t] = c[t];
	__syncthreads();
	if (threadIdx.x < 6)
	{
		const uint32_t t = threadIdx.x;
		atomicAdd(g + t * RP_SLOTS + blockIdx.x % RP_SLOTS, (unsigned long long)(s_sum[0][t] + s_sum[1][t] + s_sum[2][t] + s_sum[3][t]));
	}
}

// the block's counts into memory: every non-zero cell, which is cleared; all 256 threads
__device__ inline void report_flush(uint32_t* s_cnt, unsigned long long* __restrict__ g)
{
	__syncthreads();
	for (uint32_t c = threadIdx.x; c < RQ_CELLS + 96; c += 256)
	{
		const uint32_t v = s_cnt[c];
		if (v) { atomicAdd(g + c, (unsigned long long)v); s_cnt[c] = 0; }
	}
	__syncthreads();
}

// Blocks stride over quads of reads (quad qd = reads 4 qd .. 4 qd + 3, one wave each).  `since` = the bytes the block has counted since
// its last flush, the same in every thread: no cell can hold more, and the block flushes before a quad that would take it past
// RQ_CELL_MAX.  A quad that alone holds more is not counted and sets g[RQ_ERR] (the host refuses the call).
__global__ __launch_bounds__(256) void k_report_quals(QualValueArg cfg, const uint8_t* __restrict__ quals, const uint64_t* __restrict__ qoff, uint32_t n_reads, uint64_t flush_bytes,
                                                     unsigned long long* __restrict__ g)
{
	__shared__ uint32_t s_cnt[RQ_CELLS + 96];                                   // q_joint, then mean_q_hist
	__shared__ uint64_t s_tab8[12];
	for (uint32_t c = threadIdx.x; c < RQ_CELLS + 96; c += 256) s_cnt[c] = 0;
#pragma unroll
	for (uint32_t t = 0; t < 12; ++t) if (threadIdx.x == t) s_tab8[t] = cfg.tab8[t];
	__syncthreads();
	const uint8_t* s_tab = (const uint8_t*)s_tab8;
	const uint32_t w = threadIdx.x >> 6, lane = threadIdx.x & 63, n_quads = (n_reads + 3) / 4;
	uint64_t since = 0;
	for (uint32_t qd = blockIdx.x; qd < n_quads; qd += gridDim.x)
	{
		const uint32_t r0 = 4 * qd, r1 = n_reads - r0 < 4 ? n_reads : r0 + 4;
		const uint64_t quad_bytes = qoff[r1] - qoff[r0];                         // (block-uniform, as everything that decides a flush)
		if (quad_bytes > RQ_CELL_MAX) { if (threadIdx.x == 0) atomicAdd(g + RQ_ERR, 1ULL); continue; }
		if (since + quad_bytes > RQ_CELL_MAX) { report_flush(s_cnt, g); since = 0; }
		const uint32_t r = r0 + w;
		if (r < r1)                                                             // (wave-uniform)
		{
			const uint64_t qb = qoff[r], len = qoff[r + 1] - qb;
			uint64_t total = 0;
			qual_value_walk(cfg, s_tab, quals + qb, len, lane, [&](uint64_t v, uint64_t val, uint64_t, uint32_t nb) {
#pragma unroll
				for (uint32_t k = 0; k < 8; ++k) if (k < nb)
				{
					const uint32_t in = rp_in((uint32_t)(v >> (8 * k)) & 0xffu), out = rp_out((uint32_t)(val >> (8 * k)) & 0xffu);
					atomicAdd(&s_cnt[in * 96 + out], 1u);
					total += in;
				}
			});
			total = wave_sum64(total);
			if (lane == 0 && len) atomicAdd(&s_cnt[RQ_MEAN + rp_out((uint32_t)(total / len))], 1u);
		}
		since += quad_bytes;
		if (since >= flush_bytes) { report_flush(s_cnt, g); since = 0; }
	}
	report_flush(s_cnt, g);
}
} // namespace

extern "C" void cl_report_clear(cl_report* r) { if (r) rp_clear(r); }
extern "C" void cl_report_add(cl_report* dst, const cl_report* src) { if (dst && src) rp_add(dst, src); }

extern "C" cl_status cl_report_bases(cl_ctx* ctx, const cl_reads* R, cl_report* acc)
{
	if (!ctx || !R || !acc) return cl_fail(ctx, CL_E_INVALID, "cl_report_bases: null argument");
	if (!R->n_reads) return CL_OK;
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	DevBuf<unsigned long long> g; DEV_ALLOC(ctx, g, RB_WORDS);
	HIP_TRY(ctx, hipMemsetAsync(g.p, 0, RB_WORDS * 8, cl_launch_stream(ctx)));
	// bytes: 8 + 4 per word, i.e. 0.375 per base, and the offsets and lengths
	LAUNCHB(ctx, 12.0 * R->total_words + 12.0 * R->n_reads, k_report_bases, grid_for(R->n_reads, 4), 256, (const uint64_t*)R->packed.p, (const uint32_t*)R->inv.p,
	        (const uint64_t*)R->word_off.p, (const uint32_t*)R->lens.p, R->n_reads, g.p);
	HIP_TRY(ctx, hipGetLastError());
	unsigned long long h[RB_WORDS];
	HIP_TRY(ctx, hipMemcpyAsync(h, g.p, sizeof(h), hipMemcpyDeviceToHost, cl_launch_stream(ctx)));
	HIP_TRY(ctx, hipStreamSynchronize(cl_launch_stream(ctx)));
	cl_timing_collect(ctx);
	acc->reads += R->n_reads;
	for (uint32_t s = 0; s < RP_SLOTS; ++s)
	{
		for (uint32_t t = 0; t < 5; ++t) acc->base_count[t] += h[t * RP_SLOTS + s];
		acc->bases += h[5 * RP_SLOTS + s];
	}
	for (uint32_t b = 0; b < 33; ++b) { acc->len_hist[b] += h[RB_HIST + b]; acc->len_bases[b] += h[RB_LBASES + b]; }
	if (~h[RB_NMIN] < acc->len_min) acc->len_min = ~h[RB_NMIN];
	if (h[RB_MAX] > acc->len_max) acc->len_max = h[RB_MAX];
	return CL_OK;
}

extern "C" cl_status cl_report_quals(cl_ctx* ctx, const cl_qual_params* qparams, const cl_reads* R, const uint8_t* d_quals, const uint64_t* d_qual_off,
                                     uint64_t flush_bytes, uint32_t max_blocks, cl_report* acc)
{
	if (!ctx || !qparams || !R || !acc) return cl_fail(ctx, CL_E_INVALID, "cl_report_quals: null argument");
	if (qparams->mode == 8) return CL_OK;                                       // none: nothing is coded, nothing is counted
	DigestValueLayout V;
	if (!rp_value_layout(qparams, V)) return cl_fail(ctx, CL_E_INVALID, "cl_report_quals: mode 0..8 with the thresholds of its bins and, for *-fix, a -D value (<= 95) for every bin");
	if (R->n_reads && (!d_quals || !d_qual_off)) return cl_fail(ctx, CL_E_INVALID, "cl_report_quals: null argument");
	acc->has_qual = 1;
	if (!R->n_reads) return CL_OK;
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	if (!flush_bytes) flush_bytes = 1ULL << 30;
	if (flush_bytes > (1ULL << 32) - (1ULL << 16)) flush_bytes = (1ULL << 32) - (1ULL << 16);
	if (!max_blocks) max_blocks = 4 * (uint32_t)std::max(1, ctx->n_cu);
	const uint32_t grid = std::min(grid_for(R->n_reads, 4), max_blocks);
	QualValueArg A; A.diffuse = V.diffuse; A.bins = V.bins;
	memcpy(A.tab8, V.tab, 96);
	DevBuf<unsigned long long> g; DEV_ALLOC(ctx, g, RQ_WORDS);
	HIP_TRY(ctx, hipMemsetAsync(g.p, 0, RQ_WORDS * 8, cl_launch_stream(ctx)));
	// bytes: every quality byte once, twice where the averages need a pass of their own, and the offsets
	LAUNCHB(ctx, (V.diffuse ? 2.0 : 1.0) * R->total_bases + 8.0 * R->n_reads, k_report_quals, grid, 256, A, d_quals, d_qual_off, R->n_reads, flush_bytes, g.p);
	HIP_TRY(ctx, hipGetLastError());
	std::vector<unsigned long long> h(RQ_WORDS);
	HIP_TRY(ctx, hipMemcpyAsync(h.data(), g.p, RQ_WORDS * 8, hipMemcpyDeviceToHost, cl_launch_stream(ctx)));
	HIP_TRY(ctx, hipStreamSynchronize(cl_launch_stream(ctx)));
	cl_timing_collect(ctx);
	if (h[RQ_ERR]) return cl_fail(ctx, CL_E_UNSUPPORTED, "cl_report_quals: four consecutive reads hold 2^32 or more quality bytes");
	acc->q_reads += R->n_reads;
	for (uint32_t i = 0; i < 96; ++i)
	{
		acc->mean_q_hist[i] += h[RQ_MEAN + i];
		for (uint32_t j = 0; j < 96; ++j) { acc->q_joint[i][j] += h[i * 96 + j]; acc->q_symbols += h[i * 96 + j]; }
	}
	return CL_OK;
}

extern "C" cl_status cl_report_bases_host(const uint8_t* h_codes, const uint64_t* h_off, uint64_t n, cl_report* acc)
{
	return rp_bases_host(h_codes, h_off, n, acc) ? CL_OK : CL_E_INVALID;
}
extern "C" cl_status cl_report_quals_host(const cl_qual_params* qparams, const uint8_t* h_quals, const uint64_t* h_off, uint64_t n, cl_report* acc)
{
	return rp_quals_host(qparams, h_quals, h_off, n, acc) ? CL_OK : CL_E_INVALID;
}
extern "C" cl_status cl_report_values_host(const uint8_t* h_ascii, const uint64_t* h_off, uint64_t n, cl_report* acc)
{
	return rp_values_host(h_ascii, h_off, n, acc) ? CL_OK : CL_E_INVALID;
}

extern "C" void cl_ctx_set_report(cl_ctx* c, int on)
{
	if (!c) return;
	if (on && !c->report) { if (!c->report_acc) c->report_acc = new cl_report; rp_clear(c->report_acc); }
	c->report = on != 0;
}
extern "C" cl_status cl_ctx_report(const cl_ctx* c, cl_report* out)
{
	if (!c || !out) return CL_E_INVALID;
	if (c->report_acc) *out = *c->report_acc; else rp_clear(out);
	return CL_OK;
}
// Internal (driver.hip, stream.hip): the report of one chunk of the input into the context's total; the chunk's own report is complete
// before anything of it is added
cl_status report_chunk(cl_ctx* ctx, const cl_reads* reads, const cl_qual_params* qparams, const uint8_t* d_quals, const uint64_t* d_base_off)
{
	std::unique_ptr<cl_report> r(new cl_report);
	rp_clear(r.get());
	CL_TRY(cl_report_bases(ctx, reads, r.get()));
	if (qparams) CL_TRY(cl_report_quals(ctx, qparams, reads, d_quals, d_base_off, 0, 0, r.get()));
	rp_add(ctx->report_acc, r.get());
	return CL_OK;
}
