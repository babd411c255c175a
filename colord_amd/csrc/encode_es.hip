// encode_es.hip — kernels and host driver of the edit-script encoder (a10 + a11 + a12); the algorithm, its data
// model (frames, gaps, levels) and the reference citations are in encode_core.hpp.
//
// Per recursion level L (the loop of cl_encode_reads, <= maxRecurence + 1 iterations, each a handful of launches over ALL level-L gaps):
//   main stream: k_frame_gap_counts -> scan -> k_gap_geometry -> scans (script capacity, pending slots) -> sort by (size class, size)
//                -> k_class_bounds -> the class bounds on the host; then the aligners, side by side —
//   side:   classes 1-4, k_align_small<NB>: one lane per gap, rows <= 64 NB, columns <= 256 (Myers' recurrence in registers, sequences
//           and script in LDS, per-column history lane-interleaved in HBM)
//   side2:  class 5, k_align_quad_rows: up to 16 row blocks, four gaps per wave, banded
//   side3:  class 7, k_giant_stage / _level / _leaves / _finish: many waves per gap (align_giant.hpp)
//   main:   class 6, k_align_wave: a wave per gap on a bump pool in HBM, in rounds of growing pools (the host reads each round's redo list);
//           then the redo lists of class 5 and of class 7, read back in that order and run through the same rounds
//   main stream, when classes 1-4 are through too: k_gap_tail (a row of 16 lanes per gap: trivial scripts, estimator statistics or the static
//                entropy decision, run summary; gap_tail.hpp) -> k_gap_stats_long -> k_gap_sums_long (a wave per gap, the few scripts beyond
//                the row limit) -> k_spawn_mark -> scans -> k_spawn_fill.
// Then k_estimator (one wave per reader pack) and k_emit_count_wave / k_emit_write_wave (one wave per read; emit_wave.hpp), k_emit_plain.
#include "objects.hpp"
#include "encode_core.hpp"
#include "align_wave.hpp"
#include "align_rows.hpp"
#include "align_giant.hpp"
#include "emit_wave.hpp"
#include "gap_tail.hpp"
#include <algorithm>
#include <chrono>
#include <climits>
#include <memory>
#include <vector>

struct cl_anchors;   // anchors.hip
extern "C" const uint32_t* cl_anchors_n_cands(const cl_anchors* a);
extern "C" const uint32_t* cl_anchors_cands(const cl_anchors* a);
extern "C" const uint64_t* cl_anchors_cand_offsets(const cl_anchors* a);
extern "C" const uint32_t* cl_anchors_data(const cl_anchors* a);

using namespace enc;

namespace {
struct AnchorsV { const uint32_t* n_cands; const uint32_t* cand; const uint64_t* cand_off; const uint32_t* data; };

// ---- level 0: one frame per read that has candidates ---------------------------------------------------------------
__global__ void k_read_flags(const uint32_t* __restrict__ n_cands, const uint8_t* __restrict__ has_n, uint32_t n, uint32_t* __restrict__ flag, uint32_t* __restrict__ ncand)
{
	const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
	if (r >= n) return;
	const uint32_t nc = has_n[r] ? 0u : n_cands[r];
	flag[r] = nc ? 1u : 0u; ncand[r] = nc;
}
__global__ void k_frames_level0(ArenaV A, AnchorsV AV, uint32_t c, const uint8_t* __restrict__ has_n, uint32_t n, const uint32_t* __restrict__ frame_idx, const uint64_t* __restrict__ cand_base,
                                FrameRec* __restrict__ frames, CandEnt* __restrict__ cands, uint32_t* __restrict__ frame_of_read)
{
	const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
	if (r >= n) return;
	const uint32_t nc = has_n[r] ? 0u : AV.n_cands[r];
	if (!nc) { frame_of_read[r] = 0xffffffffu; return; }
	const uint32_t f = frame_idx[r];
	frame_of_read[r] = f;
	FrameRec F; F.read = r; F.level = 0; F.enc_off = 0; F.enc_len = A.lens[r]; F.n_cands = nc; F.first_gap = 0; F.n_gaps = 0; F.pad = 0; F.cand_base = cand_base[r];
	frames[f] = F;
	for (uint32_t j = 0; j < nc; ++j) cands[F.cand_base + j] = cand_level0(AV.cand + ((uint64_t)r * c + j) * 4, AV.cand_off[(uint64_t)r * c + j], AV.data);
}

// ---- per level ---------------------------------------------------------------------------------------------------
__global__ void k_frame_gap_counts(const FrameRec* __restrict__ frames, const CandEnt* __restrict__ cands, uint32_t n, uint32_t* __restrict__ counts)
{
	const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
	if (f < n) counts[f] = cands[frames[f].cand_base + frames[f].level].n + 1;
}
__global__ void k_frame_first_gaps(FrameRec* __restrict__ frames, const uint32_t* __restrict__ first, uint32_t n, uint32_t n_gaps)
{
	const uint32_t f = blockIdx.x * blockDim.x + threadIdx.x;
	if (f >= n) return;
	frames[f].first_gap = first[f];
	frames[f].n_gaps = (f + 1 < n ? first[f + 1] : n_gaps) - first[f];
}
__global__ void k_gap_geometry(LevelV L, ArenaV R, const uint32_t* __restrict__ data, uint32_t min_part_alt, const uint32_t* __restrict__ first_gap,
                               uint32_t* __restrict__ cap, uint32_t* __restrict__ pend_flag, uint32_t* __restrict__ keys, uint32_t* __restrict__ ids, uint32_t* __restrict__ err)
{
	const uint32_t gi = blockIdx.x * blockDim.x + threadIdx.x;
	if (gi >= L.n_gaps) return;
	uint32_t lo = 0, hi = L.n_frames;                                        // the frame that owns gap gi: last f with first_gap[f] <= gi
	while (hi - lo > 1) { const uint32_t mid = (lo + hi) >> 1; if (first_gap[mid] <= gi) lo = mid; else hi = mid; }
	GapRec g;
	if (!gap_init(L, lo, gi - first_gap[lo], data, R, g)) atomicOr(err, 4u);
	L.gaps[gi] = g;
	cap[gi] = gap_es_capacity(g);
	pend_flag[gi] = g.ne < min_part_alt ? 1u : 0u;
	keys[gi] = gap_sort_key(g);
	ids[gi] = gi;
}
__global__ void k_gap_offsets(GapRec* __restrict__ gaps, const uint64_t* __restrict__ es_off, uint32_t n)
{
	const uint32_t gi = blockIdx.x * blockDim.x + threadIdx.x;
	if (gi < n) gaps[gi].es_off = es_off[gi];
}
// bounds[N_CLASSES + 1], [N_CLASSES + 2]: over the giant gaps (class 7) the sum of their script capacities (reference + read symbols)
// in units of 256 and the largest one — what the host sizes their heap and the number of their phases by (zeroed by the caller)
__global__ void k_class_bounds(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ ids, const uint32_t* __restrict__ cap, uint32_t n, uint32_t* __restrict__ bounds /* N_CLASSES + 3 */)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i > n) return;
	if (i < n && (keys[i] >> 17) == 7) { const uint32_t c = cap[ids[i]]; atomicAdd(&bounds[N_CLASSES + 1], (c + 255) / 256); atomicMax(&bounds[N_CLASSES + 2], c); }
	const uint32_t a = i == 0 ? 0u : (keys[i - 1] >> 17) + 1, b = i == n ? N_CLASSES + 1 : (keys[i] >> 17) + 1;   // classes [a, b) start at i
	for (uint32_t c = a; c < b && c <= N_CLASSES; ++c) bounds[c] = i;
}

// algorithmic bytes of each size class: 2-bit symbols in, one script byte per symbol out — and its DP cells, rows x columns of every
// gap (what edlib's recurrence has to fill once; Hirschberg's second and third sweep over a large gap are not counted) — for the report
__global__ void k_class_bytes(const uint32_t* __restrict__ keys, const uint32_t* __restrict__ ids, const uint32_t* __restrict__ cap, const GapRec* __restrict__ gaps, uint32_t n, unsigned long long* __restrict__ bytes /* 2 x N_CLASSES */)
{
	__shared__ unsigned long long s_b[2 * N_CLASSES];
	if (threadIdx.x < 2 * N_CLASSES) s_b[threadIdx.x] = 0;
	__syncthreads();
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i < n)
	{
		uint32_t rows, cols; const uint32_t cls = gap_class(gaps[ids[i]], rows, cols);
		atomicAdd(&s_b[cls], (unsigned long long)cap[ids[i]]);
		atomicAdd(&s_b[N_CLASSES + cls], (unsigned long long)rows * cols);
	}
	__syncthreads();
	if (threadIdx.x < 2 * N_CLASSES && s_b[threadIdx.x]) atomicAdd(&bytes[threadIdx.x], s_b[threadIdx.x]);
}

// lane-private staging memory in LDS (word w of a lane at lds[w * 64 + lane]) + column history in HBM (lane-interleaved).
// PACKED: the sequences at 2 bits per symbol, the script at 4 bits per symbol (its nine letters M D A C G T X Y Z as 0..8) — 60 to 96
// words per lane (15 - 25 KB per wave) instead of 160 - 256 (40 - 64 KB with a byte per symbol, rounds 1-3: four such waves took a
// CU's whole LDS, and every other kernel that needs LDS — the sorts, the table build, the match pass — waited for them).
template<int NB>
struct LdsMem {
	static constexpr uint32_t QW = 4 * NB, TW = 16, EW = 8 * NB + 32;         // words: rows (64 NB symbols), columns (256), script (64 NB + 256 symbols)
	uint32_t* base; uint64_t* hist; uint32_t lane;
	__device__ inline uint32_t& word(uint32_t w) const { return base[w * 64 + lane]; }
	__device__ inline uint32_t q(uint32_t i) const { return (word(i >> 4) >> (2 * (i & 15))) & 3u; }
	__device__ inline uint32_t t(uint32_t j) const { return (word(QW + (j >> 4)) >> (2 * (j & 15))) & 3u; }
	__device__ inline void q_set(uint32_t i, uint32_t v) { uint32_t& w = word(i >> 4); const uint32_t sh = 2 * (i & 15); w = (w & ~(3u << sh)) | ((v & 3u) << sh); }
	__device__ inline void t_set(uint32_t j, uint32_t v) { uint32_t& w = word(QW + (j >> 4)); const uint32_t sh = 2 * (j & 15); w = (w & ~(3u << sh)) | ((v & 3u) << sh); }
	static __device__ inline uint32_t code_of(char c) { return c == 'M' ? 0u : c == 'D' ? 1u : c == 'A' ? 2u : c == 'C' ? 3u : c == 'G' ? 4u : c == 'T' ? 5u : (uint32_t)(c - 'X') + 6u; }
	static __device__ inline char char_of(uint32_t v) { return v == 0 ? 'M' : v == 1 ? 'D' : v == 2 ? 'A' : v == 3 ? 'C' : v == 4 ? 'G' : v == 5 ? 'T' : (char)('X' + (v - 6)); }
	__device__ inline char es_get(uint32_t k) const { return char_of((word(QW + TW + (k >> 3)) >> (4 * (k & 7))) & 15u); }
	__device__ inline void es_set(uint32_t k, char c) { uint32_t& w = word(QW + TW + (k >> 3)); const uint32_t sh = 4 * (k & 7); w = (w & ~(15u << sh)) | (code_of(c) << sh); }
	// script symbols 4 w .. 4 w + 3 as the four bytes of an output word
	__device__ inline uint32_t es_word(uint32_t w) const
	{
		const uint32_t x = (word(QW + TW + (w >> 1)) >> (16 * (w & 1))) & 0xffffu;
		return (uint32_t)(uint8_t)char_of(x & 15u) | ((uint32_t)(uint8_t)char_of((x >> 4) & 15u) << 8) | ((uint32_t)(uint8_t)char_of((x >> 8) & 15u) << 16) | ((uint32_t)(uint8_t)char_of(x >> 12) << 24);
	}
	__device__ inline void lap(uint32_t) {}
	__device__ inline void hist_put(uint32_t j, uint32_t b, uint64_t P, uint64_t Ph) { uint64_t* h = hist + ((uint64_t)(j * NB + b) * 2) * 64 + lane; h[0] = P; h[64] = Ph; }
	__device__ inline void hist_get(uint32_t j, uint32_t b, uint64_t& P, uint64_t& Ph) const { const uint64_t* h = hist + ((uint64_t)(j * NB + b) * 2) * 64 + lane; P = h[0]; Ph = h[64]; }
};

template<int NB>
__global__ __launch_bounds__(64) void k_align_small(const uint32_t* __restrict__ list, uint32_t n_list, GapRec* __restrict__ gaps, char* __restrict__ es_pool,
                                                   ArenaV A, ArenaV R, uint64_t* __restrict__ hist_all)
{
	extern __shared__ uint32_t lds_raw[];
	LdsMem<NB> mem{ lds_raw, hist_all + (uint64_t)blockIdx.x * (256ull * NB * 2 * 64), threadIdx.x };
	for (uint32_t chunk = blockIdx.x; (uint64_t)chunk * 64 < n_list; chunk += gridDim.x)
	{
		const uint32_t idx = chunk * 64 + threadIdx.x;
		if (idx >= n_list) continue;
		const uint32_t gi = list[idx];
		const GapRec g = gaps[gi];
		uint32_t n, m;
		stage_small(mem, g, A, R, n, m);
		uint32_t d_before;
		const uint32_t k = align_small<NB>(mem, n, m, g.kind, g.left != 0, g.nr, g.use, &d_before);
		uint32_t* dst = (uint32_t*)(es_pool + g.es_off);
		for (uint32_t w = 0; w * 4 < k; ++w) dst[w] = mem.es_word(w);
		gaps[gi].es_len = k; gaps[gi].d_before = d_before;
	}
}

// large gaps: one WAVE per gap (align_wave.hpp), largest first.  Three steps: the sequences into byte buffers (stage), sweep + path -> operations, operations -> canonical script.
struct WaveGap {
	uint8_t* rbuf; uint8_t* ebuf; uint8_t* r2; uint8_t* e2; uint8_t* opsbuf;
	const uint8_t* Q; const uint8_t* T; uint32_t n, m; bool rows_ref, shw, left;     // m: columns offered to the sweep (g.use for a flank)
};
__device__ inline bool wave_gap_stage(wv::WavePool& pool, const GapRec& g, const ArenaV& A, const ArenaV& R, WaveGap& W)
{
	const uint32_t lane = threadIdx.x & 63;
	const uint32_t ref_id = g.ref_rev & 0x7fffffffu; const bool rev = g.ref_rev >> 31;
	const uint64_t rwb = R.word_off[ref_id], ewb = A.word_off[g.read]; const uint32_t rlen = R.lens[ref_id];
	const bool left = g.left != 0;
	W.left = left;
	W.rbuf = (uint8_t*)pool.alloc(g.use + 64ull); W.ebuf = (uint8_t*)pool.alloc(g.ne + 64ull);
	W.r2 = (uint8_t*)pool.alloc(g.use + 64ull); W.e2 = (uint8_t*)pool.alloc(g.ne + 64ull);
	W.opsbuf = (uint8_t*)pool.alloc((uint64_t)g.use + g.ne + 64);
	if (pool.overflow) return false;
	const uint32_t lo = left ? g.nr - g.use : 0;
	// eight symbols per lane and step: two packed words in, one 8-byte store per buffer out (a symbol per lane was use / 64 + ne / 64 load
	// latencies in a row and four byte stores per symbol pair).  A reverse-complemented reference is read backwards: eight ascending places
	// of the stored read, bytes swapped, complemented.
	auto sym8 = [](const ArenaV& X, uint64_t wb, uint32_t fp) -> uint64_t {      // bases fp .. fp + 7 of a stored read, one per byte
		const uint64_t wa = X.packed[wb + (fp >> 5)], wz = X.packed[wb + ((fp + 7) >> 5)];
		uint64_t out = 0;
#pragma unroll
		for (uint32_t j = 0; j < 8; ++j) { const uint32_t p = fp + j; const uint64_t w = (p >> 5) == (fp >> 5) ? wa : wz; out |= ((w >> (62 - 2 * (p & 31))) & 3ull) << (8 * j); }
		return out;
	};
	auto put8 = [&](uint8_t* fwd, uint8_t* other, uint32_t total, uint32_t i, uint64_t v) {     // places i .. i + 7 of fwd; `other` is fwd or its mirror image
		__builtin_memcpy(fwd + i, &v, 8);
		if (!left) __builtin_memcpy(other + i, &v, 8);
		else { const uint64_t m = __builtin_bswap64(v); __builtin_memcpy(other + (total - 8 - i), &m, 8); }
	};
	for (uint32_t i = lane * 8; i < g.use; i += 512)
	{
		const uint32_t pos0 = g.cur_ref + lo + i;
		if (i + 8 <= g.use) put8(W.rbuf, W.r2, g.use, i, rev ? 0x0303030303030303ull - __builtin_bswap64(sym8(R, rwb, rlen - 1 - (pos0 + 7))) : sym8(R, rwb, pos0));
		else for (uint32_t y = i; y < g.use; ++y) { const uint8_t v = (uint8_t)ref_sym(R, rwb, rlen, rev, g.cur_ref + lo + y); W.rbuf[y] = v; W.r2[left ? g.use - 1 - y : y] = v; }
	}
	for (uint32_t i = lane * 8; i < g.ne; i += 512)
	{
		if (i + 8 <= g.ne) put8(W.ebuf, W.e2, g.ne, i, sym8(A, ewb, g.enc_start + i));
		else for (uint32_t y = i; y < g.ne; ++y) { const uint8_t v = (uint8_t)arena_base_at(A, ewb, g.enc_start + y); W.ebuf[y] = v; W.e2[left ? g.ne - 1 - y : y] = v; }
	}
	if (g.kind == GK_INNER) { W.Q = W.rbuf; W.n = g.nr; W.T = W.ebuf; W.m = g.ne; W.rows_ref = true; W.shw = false; }
	else if (g.kind == GK_FLANK_TINY) { W.Q = W.r2; W.n = g.use; W.T = W.e2; W.m = g.ne; W.rows_ref = true; W.shw = false; }
	else { W.Q = W.e2; W.n = g.ne; W.T = W.r2; W.m = g.use; W.rows_ref = false; W.shw = true; }
	__builtin_amdgcn_s_waitcnt(0);
	__builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
	return true;
}
__device__ inline bool wave_gap_finish(wv::WavePool& pool, GapRec& g, const WaveGap& W, const wv::Ops& ops, uint32_t ref_end, char* dst, uint32_t dbg_stage);
__device__ inline bool align_wave_gap(wv::WavePool& pool, GapRec& g, const ArenaV& A, const ArenaV& R, char* dst, uint32_t dbg_stage)
{
	g.es_len = 0; g.d_before = 0;
	WaveGap W;
	pool.beat(4);
	pool.lap(0);
	if (!wave_gap_stage(pool, g, A, R, W)) return false;
	uint8_t* const opsbuf = W.opsbuf; uint8_t* const rbuf = W.rbuf; uint8_t* const ebuf = W.ebuf; uint8_t* const r2 = W.r2; uint8_t* const e2 = W.e2;
	(void)rbuf; (void)ebuf; (void)r2; (void)e2;
	pool.beat(5);
	pool.lap(1);
	if (dbg_stage == 1) return true;
	wv::Ops ops{ opsbuf, 0 };
	const uint8_t* Q; const uint8_t* T; uint32_t n, m; uint32_t ref_end = 0;
	// when edlib would keep the whole history anyway (it decides on the truncated target, which is never longer), one
	// sweep delivers both the score / end position and the history; else score sweep first, then divide and conquer
	if (g.kind == GK_FLANK_TINY && g.use == 1 && g.ne >= 1)
	{	// ONE reference symbol against a flank of the read (seen: 1 x 121 957, 87 ms through the generic sweep + Hirschberg, the
		// slowest gap of its launch).  find_edit_dist (edit_script.h:156-239) on one row: c[1][j] = j - 1 once the symbol has
		// occurred among the first j read symbols, else j; its traceback (up, else left, else diagonal) walks left to the FIRST
		// occurrence and matches there — or, without any occurrence, substitutes the first read symbol.
		Q = r2; T = e2; n = 1; m = g.ne; ref_end = 0;
		const uint32_t lane = threadIdx.x & 63;
		const uint32_t qs = Q[0];
		uint32_t first = m;
		for (uint32_t base = 0; base < m && first == m; base += 256)
		{
			bool hit[4];
#pragma unroll
			for (uint32_t u = 0; u < 4; ++u) { const uint32_t j = base + u * 64 + lane; hit[u] = j < m && T[j] == qs; }
#pragma unroll
			for (uint32_t u = 0; u < 4; ++u) { const uint64_t bal = __ballot(hit[u]); if (bal && first == m) first = base + u * 64 + (uint32_t)__builtin_ctzll(bal); }
		}
		const uint32_t at = first < m ? first : 0; const uint8_t op_at = first < m ? 0 : 3;
		for (uint32_t j = lane; j < m; j += 64) opsbuf[j] = j == at ? op_at : 2;
		ops.n = m;
		pool.lap(2);
	}
	else if (g.kind == GK_INNER || g.kind == GK_FLANK_TINY)
	{
		if (g.kind == GK_INNER) { Q = rbuf; n = g.nr; T = ebuf; m = g.ne; }
		else { Q = r2; n = g.use; T = e2; m = g.ne; ref_end = g.use - 1; }
		if (n && m && wv::wave_direct_fits(n, m))
		{
			wv::wave_align_direct(pool, Q, n, T, m, false, ops);
			pool.lap(2);
		}
		else
		{
			const wv::Sweep sw = wv::wave_sweep(pool, Q, 1, n, wv::sat_rows(Q, 1, n, T, 1, m), T, 1, m, false, nullptr, nullptr);
			if (pool.overflow) return false;
			pool.lap(2);
			if (dbg_stage == 2) return true;
			wv::wave_path(pool, Q, n, T, m, sw.score, ops);
		}
	}
	else
	{
		Q = e2; n = g.ne; T = r2;
		if (n && g.use && wv::wave_direct_fits(n, g.use))
		{
			const wv::Sweep sw = wv::wave_align_direct(pool, Q, n, T, g.use, true, ops);
			ref_end = (uint32_t)sw.end; m = (uint32_t)(sw.end + 1);
			pool.lap(2);
		}
		else
		{
			const wv::Sweep sw = wv::wave_sweep(pool, Q, 1, n, wv::sat_rows(Q, 1, n, T, 1, g.use), T, 1, g.use, true, nullptr, nullptr);
			if (pool.overflow) return false;
			ref_end = (uint32_t)sw.end; m = (uint32_t)(sw.end + 1);
			pool.lap(2);
			if (dbg_stage == 2) return true;
			wv::wave_path(pool, Q, n, T, m, sw.best, ops);
		}
	}
	if (pool.overflow) return false;
	(void)m;
	return wave_gap_finish(pool, g, W, ops, ref_end, dst, dbg_stage);
}
// operations (0 match, 1 consume query, 2 consume target, 3 mismatch) -> the gap's canonical script
__device__ inline bool wave_gap_finish(wv::WavePool& pool, GapRec& g, const WaveGap& W, const wv::Ops& ops, uint32_t ref_end, char* dst, uint32_t dbg_stage)
{
	const uint32_t lane = threadIdx.x & 63;
	const uint8_t* const Q = W.Q; const uint8_t* const T = W.T; const bool rows_ref = W.rows_ref, left = W.left;
	const uint8_t* const rbuf = W.rbuf; const uint8_t* const ebuf = W.ebuf;
	__builtin_amdgcn_s_waitcnt(0);
	__builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
	pool.beat(6);
	pool.lap(3);
	if (dbg_stage == 3) return true;
	// operations -> script symbols, 64 at a time; for the left flank the script of the reversed sequences is written reversed
	const uint32_t k = (uint32_t)ops.n;
	// (loads run ahead of the position carries: operations two steps ahead, the sequence symbols they select one step ahead)
	{
		const uint64_t lt = lane ? (~0ull >> (64 - lane)) : 0ull;
		auto load_op = [&](uint32_t x0) -> uint32_t { const uint32_t x = x0 + lane; return x < k ? (uint32_t)ops.p[x] : 4u; };
		uint32_t opA = load_op(0), opB = load_op(64);
		uint32_t pq = 0, pt = 0, qA = 0, tA = 0;
		{
			const uint64_t cq = __ballot(opA != 2 && opA != 4), ct = __ballot(opA != 1 && opA != 4);
			const uint32_t myq = (uint32_t)__popcll(cq & lt), myt = (uint32_t)__popcll(ct & lt);
			if (opA == 1 || opA == 3) qA = Q[myq];
			if (opA == 2 || opA == 3) tA = T[myt];
			pq = (uint32_t)__popcll(cq); pt = (uint32_t)__popcll(ct);
		}
		for (uint32_t x0 = 0; x0 < k; x0 += 64)
		{
			const uint32_t x = x0 + lane;
			const uint32_t op = opA, qs = qA, ts = tA;
			const uint32_t opC = load_op(x0 + 128);
			uint32_t qB = 0, tB = 0;
			{	// the next step's symbols
				const uint64_t cq = __ballot(opB != 2 && opB != 4), ct = __ballot(opB != 1 && opB != 4);
				const uint32_t myq = pq + (uint32_t)__popcll(cq & lt), myt = pt + (uint32_t)__popcll(ct & lt);
				if (opB == 1 || opB == 3) qB = Q[myq];
				if (opB == 2 || opB == 3) tB = T[myt];
				pq += (uint32_t)__popcll(cq); pt += (uint32_t)__popcll(ct);
			}
			if (op != 4)
			{
				char ch;
				if (op == 0) ch = 'M';
				else if (op == 1) ch = rows_ref ? 'D' : base_letter(qs);
				else if (op == 2) ch = rows_ref ? base_letter(ts) : 'D';
				else ch = rows_ref ? mismatch_sym(qs, ts) : mismatch_sym(ts, qs);
				dst[left ? k - 1 - x : x] = ch;
			}
			opA = opB; opB = opC; qA = qB; tA = tB;
		}
	}
	__builtin_amdgcn_s_waitcnt(0);
	__builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
	pool.beat(7);
	pool.lap(4);
	if (dbg_stage == 4) return true;
	// canonical indel placement (wave-parallel segmented form of refactor_edit_script, align_wave.hpp)
	uint32_t d_before = 0;
	const uint8_t* rf = rbuf;
	if (left && g.kind != GK_INNER)
	{
		const uint32_t ref_offset = (g.nr - 1) - ref_end;                      // uint32 wrap for end = -1, as in the reference
		rf = rbuf + (ref_offset - (g.nr - g.use));
		d_before = ref_offset;
	}
#ifdef CL_DEBUG_REFACTOR
	char* t0 = (char*)pool.alloc(k + 64ull); char* t1 = (char*)pool.alloc(k + 64ull);
	if (pool.overflow) return false;
	for (uint32_t i = lane; i < k; i += 64) { t0[i] = dst[i]; t1[i] = dst[i]; }
	__builtin_amdgcn_s_waitcnt(0);
	__builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
	{
		struct WES { char* p; __device__ char get(uint32_t i) const { return p[i]; } __device__ void set(uint32_t i, char c) { p[i] = c; } } es{ t1 };
		refactor_es(es, k, [&](uint32_t i) -> uint32_t { return rf[i]; }, [&](uint32_t i) -> uint32_t { return ebuf[i]; });
	}
	__builtin_amdgcn_s_waitcnt(0);
	__builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
#endif
	// A flank whose read side is much longer than what is left of the reference read ends (right flank) or starts (left flank:
	// the script of the reversed sequences is written reversed) in ONE run of inserted letters as long as the excess — the rows
	// the sweeps leave out (wv::sat_rows).  Both passes are the identity on such a run: pass 1 breaks at every insertion, and a
	// pass-2 region without a match is rewritten as itself.  A pass-2 region may reach into the run as far as the run's first
	// (last) letter repeats, so the passes look at the rest of the script plus that stretch — not at 10^5 letters.
	uint32_t ra = 0, rb = k;
	if (k >= 256)
	{
		auto is_ins = [](char c) { return c == 'A' || c == 'C' || c == 'G' || c == 'T'; };
		uint32_t b0 = k;                                                        // start of the maximal suffix of inserted letters
		while (b0 > 0)
		{
			const uint32_t lo = b0 >= 64 ? b0 - 64 : 0, x = lo + lane;
			const uint64_t non = __ballot(x < b0 && !is_ins(dst[x]));
			if (non) { b0 = lo + (63 - (uint32_t)__builtin_clzll(non)) + 1; break; }
			b0 = lo;
		}
		if (b0 < k)
		{	// ... plus the stretch over which its first letter repeats
			const char c0 = dst[b0];
			rb = k;
			for (uint32_t x0 = b0; x0 < k; x0 += 64)
			{
				const uint32_t x = x0 + lane;
				const uint64_t dif = __ballot(x < k && dst[x] != c0);
				if (dif) { rb = x0 + (uint32_t)__builtin_ctzll(dif); break; }
			}
		}
		uint32_t a0 = 0;                                                        // length of the maximal prefix of inserted letters
		for (; a0 < rb; )
		{
			const uint32_t x = a0 + lane;
			const uint64_t non = __ballot(x < rb && !is_ins(dst[x]));
			if (non) { a0 += (uint32_t)__builtin_ctzll(non); break; }
			a0 = a0 + 64 < rb ? a0 + 64 : rb;
		}
		if (a0 >= rb) ra = rb;                                                  // nothing but insertions: both passes are the identity
		else if (a0 > 0)
		{	// ... minus the stretch over which its last letter repeats
			const char c1 = dst[a0 - 1];
			ra = 0;
			for (uint32_t hi = a0; hi > 0; )
			{
				const uint32_t lo = hi >= 64 ? hi - 64 : 0, x = lo + lane;
				const uint64_t dif = __ballot(x < hi && dst[x] != c1);
				if (dif) { ra = lo + (63 - (uint32_t)__builtin_clzll(dif)) + 1; break; }
				hi = lo;
			}
		}
	}
	// (the skipped prefix consumes no reference symbol and `ra` read symbols)
	if (rb > ra && !wv::wave_refactor(pool, dst + ra, rb - ra, rf, ebuf + ra)) return false;
#ifdef CL_DEBUG_REFACTOR
	if (lane == 0)
	{
		uint32_t bad = k;
		for (uint32_t i = 0; i < k; ++i) if (dst[i] != t1[i]) { bad = i; break; }
		if (bad < k)
		{
			const uint32_t lo = bad > 70 ? bad - 70 : 0;
			printf("refactor mismatch k=%u at %u (lo %u)\n in : %.100s\n exp: %.100s\n got: %.100s\n", k, bad, lo, t0 + lo, t1 + lo, dst + lo);
		}
	}
#endif
	g.es_len = k; g.d_before = d_before;
	pool.lap(5);
	return true;
}
__global__ __launch_bounds__(64) void k_align_wave(const uint32_t* __restrict__ list, uint32_t n_list, GapRec* __restrict__ gaps, char* __restrict__ es_pool, ArenaV A, ArenaV R,
                                                  uint8_t* __restrict__ scratch, uint64_t per_wave, unsigned int* __restrict__ next, uint32_t* __restrict__ redo, unsigned int* __restrict__ n_redo, uint32_t dbg_stage, uint32_t* hbt, unsigned long long* prof)
{
	__builtin_amdgcn_s_setprio(3);                                          // a launch of this kernel lasts as long as its slowest chain: its waves go first on their SIMDs
	wv::WavePool pool{ scratch + (uint64_t)blockIdx.x * per_wave, per_wave, 0, false, hbt ? hbt + blockIdx.x : nullptr };
	pool.prof = prof; if (prof) pool.t_last = wall_clock64();
	pool.beat(1);
	const uint32_t lane = threadIdx.x;
	for (;;)
	{	// the list is ascending in size: the waves draw from its end, largest first, whenever they are free (a wave that got one
		// of the few huge gaps takes no further share of the rest)
		uint32_t slot = 0;
		if (lane == 0) slot = atomicAdd(next, 1u);
		slot = wv::bcast_first(slot);
		if (slot >= n_list) break;
		pool.beat(2);
		const uint32_t gi = list[n_list - 1 - slot];
		pool.top = 0; pool.overflow = false;
		GapRec g = gaps[gi];
		pool.beat(3);
		pool.lap(7);
		const uint64_t t_gap = prof ? wall_clock64() : 0;
		if (prof) for (int i = 0; i < 8; ++i) pool.gp[i] = 0;
		const bool ok_gap = align_wave_gap(pool, g, A, R, es_pool + g.es_off, dbg_stage);
		if (prof && lane == 0)
		{	// (diagnostic: the slowest gap, its rank, shape and phases)
			const unsigned long long mine = ((unsigned long long)(wall_clock64() - t_gap) << 24) | (slot & 0xffffffu);
			if (atomicMax(prof + 6, mine) < mine) { for (int i = 0; i < 6; ++i) prof[8 + i] = pool.gp[i]; prof[14] = ((unsigned long long)g.ne << 32) | g.use; prof[15] = g.kind; }
		}
		if (!ok_gap)
		{
			if (lane == 0) redo[atomicAdd(n_redo, 1u)] = gi;
			continue;
		}
		pool.beat(8);
		if (lane == 0) { gaps[gi].es_len = g.es_len; gaps[gi].d_before = g.d_before; }
	}
	pool.beat(9);
}

// giant gaps: MANY waves per gap (align_giant.hpp): phases of tile jobs over all giants of the level — score sweeps, then Hirschberg
// level by level —, then the leaves' tracebacks, then operations -> canonical script per gap.  What fails (capacities, heap, a
// hand-over that never came) goes to `redo` and the wave-per-gap kernel.
__global__ __launch_bounds__(256) void k_giant_stage(gt::View V, const uint32_t* __restrict__ list, const GapRec* __restrict__ gaps, ArenaV A, ArenaV R)
{
	__shared__ gt::Giant sg;
	const uint32_t gidx = blockIdx.x, tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
	const GapRec g = gaps[list[V.n_giants - 1 - gidx]];                       // ascending by work: largest first
	const bool left = g.left != 0;
	if (w == 0)
	{
		uint8_t* rbuf = gt::galloc(V, g.use + 64ull); uint8_t* ebuf = gt::galloc(V, g.ne + 64ull);
		uint8_t* r2 = gt::galloc(V, g.use + 64ull); uint8_t* e2 = gt::galloc(V, g.ne + 64ull);
		uint8_t* opsbuf = gt::galloc(V, (uint64_t)g.use + g.ne + 64); uint8_t* sparse = gt::galloc(V, (uint64_t)g.use + g.ne + 64);
		if (lane == 0)
		{
			gt::Giant G; memset(&G, 0, sizeof(G));
			G.gi = list[V.n_giants - 1 - gidx]; G.kind = g.kind; G.left = left ? 1u : 0u;
			G.fail = (rbuf && ebuf && r2 && e2 && opsbuf && sparse) ? 0u : 12u;
			G.rbuf = rbuf; G.ebuf = ebuf; G.r2 = r2; G.e2 = e2; G.opsbuf = opsbuf; G.sparse = sparse;
			if (g.kind == GK_INNER) { G.Q = rbuf; G.n = g.nr; G.T = ebuf; G.m = g.ne; G.rows_ref = 1; G.shw = 0; }
			else if (g.kind == GK_FLANK_TINY) { G.Q = r2; G.n = g.use; G.T = e2; G.m = g.ne; G.rows_ref = 1; G.shw = 0; G.ref_end_nw = g.use - 1; }
			else { G.Q = e2; G.n = g.ne; G.T = r2; G.m = g.use; G.rows_ref = 0; G.shw = 1; }
			sg = G;
		}
	}
	__syncthreads();
	if (sg.fail) { if (tid == 0) V.giants[gidx] = sg; return; }
	{
		const uint32_t ref_id = g.ref_rev & 0x7fffffffu; const bool rev = g.ref_rev >> 31;
		const uint64_t rwb = R.word_off[ref_id], ewb = A.word_off[g.read]; const uint32_t rlen = R.lens[ref_id];
		const uint32_t lo = left ? g.nr - g.use : 0;
		for (uint32_t i = tid; i < g.use; i += 256) { const uint8_t v = (uint8_t)ref_sym(R, rwb, rlen, rev, g.cur_ref + lo + i); sg.rbuf[i] = v; sg.r2[left ? g.use - 1 - i : i] = v; }
		for (uint32_t i = tid; i < g.ne; i += 256) { const uint8_t v = (uint8_t)arena_base_at(A, ewb, g.enc_start + i); sg.ebuf[i] = v; sg.e2[left ? g.ne - 1 - i : i] = v; }
		for (uint64_t x = tid; x < (uint64_t)g.use + g.ne; x += 256) sg.sparse[x] = 0xff;
	}
	__syncthreads();
	if (w != 0) return;
	if (lane == 0) V.giants[gidx] = sg;
	__builtin_amdgcn_s_waitcnt(0);
	__builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
	// the score (and, for a flank, where the alignment ends in the reference): a sweep of phase 0 — or closed form when the rows saturate
	const uint32_t n = sg.n, mc = sg.m;
	const uint32_t ne = wv::sat_rows(sg.Q, 1, n, sg.T, 1, mc);
	if (ne < n)
	{
		const uint32_t mp = mc, ref_end = sg.shw ? mc - 1 : sg.ref_end_nw;        // D[n][j] = n - j falls strictly: the first minimum is the last column
		if (lane == 0) { V.giants[gidx].mp = mp; V.giants[gidx].ref_end = ref_end; }
		gt::emit_sub(V, gidx, 0, n, 0, mp, n - mc, 1);
		return;
	}
	const uint32_t tiles = ((ne + 63) / 64 + 63) / 64, chunks = (mc + 63) / 64;
	unsigned long long* hand = tiles > 1 ? (unsigned long long*)gt::galloc(V, (uint64_t)(tiles - 1) * chunks * 16) : nullptr;
	const uint32_t f0 = gt::take(&V.ctl->n_flags, tiles - 1);
	const uint32_t ni = gt::take(&V.ctl->n_nodes[0], 1), si = gt::take(&V.ctl->n_sweeps[0], 1), ji = gt::take(&V.ctl->n_jobs[0], tiles);
	if ((tiles > 1 && !hand) || f0 + tiles - 1 > gt::FLAG_CAP || ni >= gt::NODE_CAP || si >= 2 * gt::NODE_CAP || ji + tiles > gt::JOB_CAP)
	{
		for (uint32_t x = lane; x < tiles; x += 64) if (ji + x < gt::JOB_CAP) V.jobs[0][ji + x] = gt::Job{ 0xffffffffu, 0 };
		gt::giant_fail(V, gidx, 13);
		return;
	}
	if (lane == 0)
	{
		V.nodes[0][ni] = gt::Node{ gidx, 0, n, 0, mc, 0, 0, 0, 0, 0, nullptr, nullptr, tiles, si };
		V.sweeps[0][si] = gt::Sweep{ sg.Q, sg.T, 1, 1, n, ne, mc, sg.shw, nullptr, hand, V.flags + f0, tiles, ni, 0, 0, 0, 0 };
	}
	for (uint32_t x = lane; x < tiles; x += 64) V.jobs[0][ji + x] = gt::Job{ si, x };
}
__global__ __launch_bounds__(64) void k_giant_level(gt::View V, uint32_t ph)
{
	__builtin_amdgcn_s_setprio(3);
	const uint32_t lane = threadIdx.x;
	const uint32_t n_jobs = V.ctl->n_jobs[ph] < gt::JOB_CAP ? V.ctl->n_jobs[ph] : gt::JOB_CAP;
	for (;;)
	{
		const uint32_t ticket = gt::take(&V.ctl->ticket[ph], 1);
		if (ticket >= n_jobs) break;
		const gt::Job jb = V.jobs[ph & 1][ticket];
		if (jb.sweep == 0xffffffffu) continue;
		gt::Sweep* S = &V.sweeps[ph & 1][jb.sweep];
		gt::Node* N = &V.nodes[ph & 1][S->node];
		const uint32_t giant = N->giant;
		if (!gt::giant_tile(S, jb.tile)) gt::giant_fail(V, giant, 14);
		// the node's last tile splits it: what the other tiles wrote (their parts of the last columns, the sweep's result) is released
		// before the count-down and acquired after it
		__threadfence();
		uint32_t left = 1;
		if (lane == 0) left = atomicSub(&N->pending, 1u) - 1;
		left = wv::bcast_first(left);
		if (left) continue;
		__threadfence();
		if (V.giants[giant].fail) continue;
		if (ph == 0)
		{
			const gt::Giant& G = V.giants[giant];
			const uint32_t score = wv::bcast_first(S->score), best = wv::bcast_first(S->best); const int32_t end = (int32_t)wv::bcast_first((uint32_t)S->end);
			const uint32_t mp = G.shw ? (uint32_t)(end + 1) : G.m, ref_end = G.shw ? (uint32_t)end : G.ref_end_nw;
			if (lane == 0) { V.giants[giant].mp = mp; V.giants[giant].ref_end = ref_end; }
			gt::emit_sub(V, giant, 0, G.n, 0, mp, G.shw ? best : score, 1);
		}
		else
		{
			const gt::Node nd = *N;
			uint32_t ls = 0, rs = 0;
			const int64_t found = wv::hirschberg_split(nd.left, nd.neL, nd.L, nd.right, nd.neR, nd.R, nd.n, nd.best, ls, rs);
			if (found < 0) { gt::giant_fail(V, giant, 15); continue; }
			gt::emit_sub(V, giant, nd.qo, (uint32_t)found, nd.to, nd.L, ls, ph + 1);
			gt::emit_sub(V, giant, nd.qo + (uint32_t)found, nd.n - (uint32_t)found, nd.to + nd.L, nd.R, rs, ph + 1);
		}
	}
}
__global__ __launch_bounds__(64) void k_giant_leaves(gt::View V, uint8_t* __restrict__ scratch, uint64_t per_wave)
{
	__builtin_amdgcn_s_setprio(3);
	wv::WavePool pool{ scratch + (uint64_t)blockIdx.x * per_wave, per_wave, 0, false, nullptr };
	const uint32_t lane = threadIdx.x;
	const uint32_t n_leaves = V.ctl->n_leaves < gt::LEAF_CAP ? V.ctl->n_leaves : gt::LEAF_CAP;
	for (;;)
	{
		const uint32_t ticket = gt::take(&V.ctl->leaf_ticket, 1);
		if (ticket >= n_leaves) break;
		const gt::Leaf lf = V.leaves[ticket];
		const gt::Giant& G = V.giants[lf.giant];
		if (G.fail) continue;
		uint8_t* dst = G.sparse + lf.qo + lf.to;                                // sub-problems tile the alignment in this order; n x m symbols give at most n + m operations
		if (lf.n == 0 || lf.m == 0)
		{
			const uint8_t op = lf.n == 0 ? 2 : 1;
			for (uint64_t x = lane; x < (uint64_t)lf.n + lf.m; x += 64) dst[x] = op;
			continue;
		}
		pool.top = 0; pool.overflow = false;
		wv::Ops o{ dst, 0 };
		wv::wave_traceback(pool, G.Q + lf.qo, lf.n, G.T + lf.to, lf.m, o);
		if (pool.overflow) gt::giant_fail(V, lf.giant, 16);
	}
}
__global__ __launch_bounds__(64) void k_giant_finish(gt::View V, GapRec* __restrict__ gaps, char* __restrict__ es_pool, uint8_t* __restrict__ scratch, uint64_t per_wave,
                                                    unsigned int* __restrict__ next, uint32_t* __restrict__ redo, unsigned int* __restrict__ n_redo)
{
	__builtin_amdgcn_s_setprio(3);
	wv::WavePool pool{ scratch + (uint64_t)blockIdx.x * per_wave, per_wave, 0, false, nullptr };
	const uint32_t lane = threadIdx.x;
	for (;;)
	{
		const uint32_t gidx = gt::take(next, 1);
		if (gidx >= V.n_giants) break;
		const gt::Giant G = V.giants[gidx];
		bool done = false;
		GapRec g = gaps[G.gi];
		if (!G.fail)
		{	// the sparse buffer -> the operations, in order (a chunk of 64 at a time, the offset carried along)
			const uint64_t span = (uint64_t)G.n + G.mp;
			uint64_t off = 0;
			for (uint64_t x0 = 0; x0 < span; x0 += 64)
			{
				const uint64_t x = x0 + lane;
				const uint8_t v = x < span ? G.sparse[x] : (uint8_t)0xff;
				const uint64_t bal = __ballot(v != 0xff);
				if (v != 0xff) G.opsbuf[off + (uint32_t)__popcll(bal & ((1ull << lane) - 1))] = v;
				off += (uint32_t)__popcll(bal);
			}
			__builtin_amdgcn_s_waitcnt(0);
			__builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
			WaveGap W; W.rbuf = G.rbuf; W.ebuf = G.ebuf; W.r2 = G.r2; W.e2 = G.e2; W.opsbuf = G.opsbuf; W.Q = G.Q; W.T = G.T; W.n = G.n; W.m = G.m;
			W.rows_ref = G.rows_ref != 0; W.shw = G.shw != 0; W.left = G.left != 0;
			wv::Ops ops{ G.opsbuf, off };
			pool.top = 0; pool.overflow = false;
			g.es_len = 0; g.d_before = 0;
			done = wave_gap_finish(pool, g, W, ops, G.ref_end, es_pool + g.es_off, 0);
		}
		if (lane == 0)
		{
			if (done) { gaps[G.gi].es_len = g.es_len; gaps[G.gi].d_before = g.d_before; }
			else redo[atomicAdd(n_redo, 1u)] = G.gi;
		}
	}
}

// gaps of up to 16 row blocks (rows <= 1024, rows + columns <= 2048): FOUR per wave, every phase of a gap in its 16-lane row (align_rows.hpp;
// round 5): sequences, operations and script in LDS, the banded history in the wave's pool.  What does not fit (pool, LDS, a distance beyond the
// band) goes to `redo` (k_align_wave takes it).  Rounds 2-4 ran only the sweep four gaps at a time (k_align_quad_hist: 495 us per quad against
// 233 here; a form without history in HBM — checkpoints, windows recomputed into LDS — was 1.25 x slower still: numbers in DESIGN.md).
// PROF (COLORD_HIP_QUAD_PROFILE): 100-MHz clocks per phase and the traceback's window statistics, summed over the waves into prof[0..10]
template<bool PROF>
__global__ __launch_bounds__(64) void k_align_quad_rows(const uint32_t* __restrict__ list, uint32_t n_list, GapRec* __restrict__ gaps, char* __restrict__ es_pool, ArenaV A, ArenaV R,
                                                  uint8_t* __restrict__ scratch, uint64_t per_wave, unsigned int* __restrict__ next, uint32_t* __restrict__ redo, unsigned int* __restrict__ n_redo, unsigned long long* __restrict__ prof)
{
	uint64_t t_last = PROF ? wall_clock64() : 0;
	auto lap = [&](uint32_t phase) { if (PROF) { const uint64_t now = wall_clock64(); if (threadIdx.x == 0) atomicAdd(prof + phase, (unsigned long long)(now - t_last)); t_last = now; } };
	qr::WalkStats wstat;
	__shared__ __attribute__((aligned(16))) uint8_t s_rows[4 * qr::ROW_BYTES];
	const uint32_t lane = threadIdx.x, gq = lane >> 4, bl = lane & 15;
	ulonglong2* const pool = (ulonglong2*)(scratch + (uint64_t)blockIdx.x * per_wave);
	const uint64_t pool_pairs = per_wave / 16;
	const uint32_t n_quads = (n_list + 3) / 4;
	uint8_t* const mem = s_rows + gq * qr::ROW_BYTES;
	for (;;)
	{
		uint32_t slot = 0;
		if (lane == 0) slot = atomicAdd(next, 1u);
		slot = wv::bcast_first(slot);
		if (slot >= n_quads) break;
		const uint32_t hi = n_list - slot * 4, cnt = hi < 4 ? hi : 4;            // gaps list[hi - 1], list[hi - 2], ... (ascending list, taken from its end)
		const bool have = gq < cnt;
		const uint32_t gi = have ? list[hi - 1 - gq] : 0u;
		GapRec g; memset(&g, 0, sizeof(g));
		if (have) g = gaps[gi];
		qr::Row r;
		r.seq = (uint32_t*)mem; r.ops = mem + qr::SEQ_WORDS * 4; r.es = r.ops + qr::SEQ_MAX;
		r.use = g.use; r.ne = g.ne; r.e_off = (g.use + 15) / 16;
		r.left = g.left != 0; r.rev_seq = r.left && g.kind != GK_INNER;
		if (g.kind == GK_INNER) { r.n = g.nr; r.m = g.ne; r.rows_ref = true; r.shw = false; }
		else if (g.kind == GK_FLANK_TINY) { r.n = g.use; r.m = g.ne; r.rows_ref = true; r.shw = false; }
		else { r.n = g.ne; r.m = g.use; r.rows_ref = false; r.shw = true; }
		const uint32_t nb = (r.n + 63) / 64;
		const uint64_t pairs = (uint64_t)qr::hist_stride(r.m) * nb;
		// what the sweep keeps of its history: the blocks within `band` rows of a column (align_rows.hpp); a distance beyond it: not of this kernel
		const uint32_t band = (r.shw ? r.n : (r.n > r.m ? r.n : r.m)) / 4 + 16;
		bool ok = have && r.n && r.m && r.n <= 1024 && (g.kind != GK_INNER || g.nr == g.use) && g.use + g.ne <= qr::SEQ_MAX;
		// the rows' shares of the pool (a row that does not fit takes none)
		uint64_t off = 0;
		{
			const uint64_t mine = ok ? pairs : 0;
			const uint64_t p0 = wv::bcast(mine, 0u), p1 = wv::bcast(mine, 16u), p2 = wv::bcast(mine, 32u);
			off = gq == 0 ? 0 : gq == 1 ? p0 : gq == 2 ? p0 + p1 : p0 + p1 + p2;
			if (off + mine > pool_pairs) ok = false;
		}
		if (!ok) { r.n = 0; r.m = 0; }
		ulonglong2* const hist = pool + off;
		lap(5);
		qr::row_stage(r, ok, g, A, R);
		qr::lds_fence();
		lap(0);
		const wv::Sweep sw = qr::row_sweep(r, hist, band);
		__builtin_amdgcn_s_waitcnt(0);
		__builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
		if (ok && (r.shw ? sw.best : sw.score) > band) { ok = false; r.n = 0; r.m = 0; }
		lap(1);
		uint32_t wi, wj, wk;
		qr::row_walk(r, hist, r.shw ? (uint32_t)(sw.end + 1) : r.m, wi, wj, wk, PROF ? &wstat : nullptr);
		qr::lds_fence();
		lap(2);
		const uint32_t pre = wi + wj, K = pre + wk;
		qr::row_convert(r, pre, (uint8_t)(wi ? 1 : 2), wk);
		qr::lds_fence();
		lap(3);
		// canonical indel placement: pass 1 along the reference symbols the script consumes, pass 2 along the read's
		const uint32_t ref_end = r.shw ? (uint32_t)sw.end : g.kind == GK_FLANK_TINY ? g.use - 1 : 0u;
		uint32_t d_before = 0, seq_off = 0;
		if (r.left && g.kind != GK_INNER)
		{
			const uint32_t ref_offset = (g.nr - 1) - ref_end;                    // uint32 wrap for end = -1, as in the reference
			seq_off = ref_offset - (g.nr - g.use);
			d_before = ref_offset;
		}
		qr::row_refactor_pass(r, K, seq_off, 1);
		qr::row_refactor_pass(r, K, 0, 2);
		lap(4);
		if (ok)
		{
			uint32_t* dst = (uint32_t*)(es_pool + g.es_off); const uint32_t* src = (const uint32_t*)r.es;
			for (uint32_t w = bl; w * 4 < K; w += 16) dst[w] = src[w];
		}
		if (have && bl == 0)
		{
			if (ok) { gaps[gi].es_len = K; gaps[gi].d_before = d_before; }
			else redo[atomicAdd(n_redo, 1u)] = gi;
		}
		qr::lds_fence();
		if (PROF) { const uint32_t smax = qr::max4(r.n ? r.m + nb - 1 : 0); if (lane == 0) { atomicAdd(prof + 9, 1ull); atomicAdd(prof + 10, (unsigned long long)smax); } }
	}
	if (PROF && lane == 0) { atomicAdd(prof + 6, (unsigned long long)wstat.iters); atomicAdd(prof + 7, (unsigned long long)wstat.miss); atomicAdd(prof + 8, (unsigned long long)wstat.hit); }
}

// (no lane-per-gap kernel: align_large (align_dev.hpp) and align_large_gap (encode_core.hpp) stay as the reference that
// tests/tools/encode_host.hip compiles for the host and the device aligners are compared with)

// the tail of a level (gap_tail.hpp): trivial scripts, estimator statistics or the static entropy decision, the spawn flag and the run
// summary of every gap in one pass over its script.  One 16-lane ROW per gap, four gaps per wave, taken through the list sorted by class
// and size, so that the rows of a wave hold scripts of similar length.  A script beyond row_limit symbols is listed for the two
// whole-wave kernels below (the order of that list decides nothing)
__global__ __launch_bounds__(256) void k_gap_tail(LevelV L, ArenaV A, EncCfg cfg, const uint32_t* __restrict__ ids, const uint32_t* __restrict__ pend_idx, GapSum* __restrict__ sums,
                                                  uint32_t* __restrict__ spawn_flag, uint32_t row_limit, uint32_t* __restrict__ over_ids, unsigned int* __restrict__ n_over)
{
	const uint64_t ri = ((uint64_t)blockIdx.x * 256 + threadIdx.x) >> 4;
	if (ri >= L.n_gaps) return;
	const uint32_t gi = ids[ri];
	const GapRec g = L.gaps[gi];
	const uint32_t k = g.kind == GK_TRIVIAL && g.nr == 0 ? g.ne : g.es_len;       // a trivial gap's script is made here
	if (k > row_limit) { if ((threadIdx.x & 15) == 0) over_ids[atomicAdd(n_over, 1u)] = gi; return; }
	gap_tail_group<16, true>(L, A, cfg, gi, g, pend_idx[gi], sums, spawn_flag);      // pend_idx = number of short gaps before gi
}
// ... the listed gaps by a wave each: statistics / decision (their run summaries: k_gap_sums_long, which reads the script lengths set here)
__global__ __launch_bounds__(256) void k_gap_stats_long(LevelV L, ArenaV A, EncCfg cfg, const uint32_t* __restrict__ pend_idx, const uint32_t* __restrict__ over_ids,
                                                        const unsigned int* __restrict__ n_over, uint32_t* __restrict__ spawn_flag)
{
	const uint32_t n = *n_over, n_waves = gridDim.x * 4;
	for (uint32_t idx = blockIdx.x * 4 + (threadIdx.x >> 6); idx < n; idx += n_waves)
	{
		const uint32_t gi = over_ids[idx];
		gap_tail_group<64, false>(L, A, cfg, gi, L.gaps[gi], pend_idx[gi], nullptr, spawn_flag);
	}
}
// ... and their run summaries (the wave-per-read emission works from summaries alone; a lane would take a millisecond for the 10^5
// symbols of a long flank and hold its launch that long)
__global__ __launch_bounds__(256) void k_gap_sums_long(LevelV L, GapSum* __restrict__ sums, const uint32_t* __restrict__ long_ids, const unsigned int* __restrict__ n_long)
{
	const uint32_t n = *n_long, n_waves = gridDim.x * 4;
	for (uint32_t idx = blockIdx.x * 4 + (threadIdx.x >> 6); idx < n; idx += n_waves)
	{
		const uint32_t gi = long_ids[idx];
		const RunEl a = run_of_script_wave(L.es + L.gaps[gi].es_off, L.gaps[gi].es_len);
		if ((threadIdx.x & 63) == 0) sums[gi] = GapSum{ a.hl, a.tl, a.mb, a.mt, a.hs | (a.ts << 8) | (a.single ? 1u << 16 : 0u) };
	}
}
// rejected long gaps: continue in a child frame when an alternative candidate still has anchors there, else literal
__global__ void k_spawn_mark(LevelV L, const uint32_t* __restrict__ data, EncCfg cfg, uint32_t* __restrict__ flag, uint32_t* __restrict__ ncand)
{
	const uint32_t gi = blockIdx.x * blockDim.x + threadIdx.x;
	if (gi >= L.n_gaps) return;
	ncand[gi] = 0;
	if (!flag[gi]) return;
	const GapRec g = L.gaps[gi];
	const FrameRec F = L.frames[g.frame];
	CandEnt out[16];
	const bool alt = spawn_cands(F, L.cands + F.cand_base, data, g, cfg, out);
	flag[gi] = alt ? 1u : 0u;
	ncand[gi] = alt ? F.n_cands : 0u;
	if (!alt) L.gaps[gi].state = GS_LITERAL;
}
__global__ void k_spawn_fill(LevelV L, const uint32_t* __restrict__ data, EncCfg cfg, const uint32_t* __restrict__ flag_scan, const uint64_t* __restrict__ cand_base,
                             FrameRec* __restrict__ frames_next, CandEnt* __restrict__ cands_next)
{
	const uint32_t gi = blockIdx.x * blockDim.x + threadIdx.x;
	if (gi >= L.n_gaps) return;
	if (cand_base[gi + 1] == cand_base[gi]) return;
	spawn_child(L, gi, data, cfg, flag_scan[gi], cand_base[gi], frames_next, cands_next);
}

// ---- estimator and emission -------------------------------------------------------------------------------------------
__global__ void k_read_base_counts(ArenaV A, const uint8_t* __restrict__ has_n, uint32_t n, uint32_t* __restrict__ counts /* 4 per read */)
{	// one wave per read
	const uint32_t r = (blockIdx.x * blockDim.x + threadIdx.x) >> 6, lane = threadIdx.x & 63;
	if (r >= n) return;
	uint32_t c0 = 0, c1 = 0, c2 = 0, c3 = 0;
	if (!has_n[r])
	{
		const uint32_t len = A.lens[r]; const uint64_t wb = A.word_off[r];
		for (uint32_t w = lane; w * 32 < len; w += 64)
		{
			const uint64_t x = A.packed[wb + w]; const uint32_t cnt = len - w * 32 < 32 ? len - w * 32 : 32;
			const uint64_t lo = x & 0x5555555555555555ull, hi = (x >> 1) & 0x5555555555555555ull;
			const uint64_t valid = cnt == 32 ? 0x5555555555555555ull : (0x5555555555555555ull & ~((1ull << (64 - 2 * cnt)) - 1));
			c0 += __popcll(~hi & ~lo & valid); c1 += __popcll(~hi & lo & valid); c2 += __popcll(hi & ~lo & valid); c3 += __popcll(hi & lo & valid);
		}
	}
	for (int o = 32; o; o >>= 1) { c0 += __shfl_xor(c0, o); c1 += __shfl_xor(c1, o); c2 += __shfl_xor(c2, o); c3 += __shfl_xor(c3, o); }
	if (lane == 0) { counts[4 * r] = c0; counts[4 * r + 1] = c1; counts[4 * r + 2] = c2; counts[4 * r + 3] = c3; }
}
// events of the estimator: the pending gaps of every read in encoding order (depth-first over its frames)
__global__ void k_pend_count(TreeV T, uint32_t n_reads, uint32_t* __restrict__ cnt)
{
	const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
	if (r >= n_reads) return;
	const uint32_t f0 = T.frame_of_read[r];
	cnt[r] = f0 == 0xffffffffu ? 0u : pend_walk(T, f0, nullptr);
}
__global__ void k_pend_list(TreeV T, uint32_t n_reads, const uint64_t* __restrict__ off, uint32_t* __restrict__ events)
{
	const uint32_t r = blockIdx.x * blockDim.x + threadIdx.x;
	if (r >= n_reads) return;
	const uint32_t f0 = T.frame_of_read[r];
	if (f0 != 0xffffffffu && off[r + 1] > off[r]) pend_walk(T, f0, events + off[r]);
}
// CEntropyEstimator over one reader pack by one wave (utils.h:877-1130): the events are inherently sequential, the work
// inside one event is not — lanes 0..11 hold the 12 edit-script counters and take the logarithms in parallel, lanes
// 12..15 precompute the decision logarithms of both outcomes; sums are then accumulated in the reference's order.
__global__ __launch_bounds__(64) void k_estimator(TreeV T, const uint32_t* __restrict__ pack_bounds, uint32_t n_packs, const uint32_t* __restrict__ lens, const uint8_t* __restrict__ has_n,
                                                 const uint32_t* __restrict__ base_counts, const uint64_t* __restrict__ ev_off, const uint32_t* __restrict__ events)
{
	__builtin_amdgcn_s_setprio(3);                                          // a launch of this kernel lasts as long as its slowest chain: its waves go first on their SIMDs
	__shared__ PendRec recs[64];
	__shared__ uint32_t ev_id[64];
	const uint32_t pk = blockIdx.x, lane = threadIdx.x;
	if (pk >= n_packs) return;
	const uint32_t MX = 1u << 20;
	uint32_t es_l = lane < 12 ? 1u : 0u, es_sum = 12;
	uint32_t dna0 = 1, dna1 = 1, dna2 = 1, dna3 = 1, dna_sum = 4, dec0 = 1, dec1 = 1, dec_sum = 2;
	double dl0, dl1, dl2, dl3, dcl0, dcl1;
	{ const double r4 = 1.0 / 4, r2 = 1.0 / 2; dl0 = dl1 = dl2 = dl3 = -glibc_log2::log2(1.0 * r4); dcl0 = dcl1 = -glibc_log2::log2(1.0 * r2); }
	for (uint32_t r = pack_bounds[pk]; r < pack_bounds[pk + 1]; ++r)
	{
		if (has_n[r]) continue;                                                  // reads with N never reach the estimator (encoder.cpp:1629-1633)
		{	// LogRead (utils.h:946-955)
			dna0 += base_counts[4 * r]; dna1 += base_counts[4 * r + 1]; dna2 += base_counts[4 * r + 2]; dna3 += base_counts[4 * r + 3];
			dna_sum += lens[r];
			while (dna_sum > MX) { dna0 = (dna0 + 1) / 2; dna1 = (dna1 + 1) / 2; dna2 = (dna2 + 1) / 2; dna3 = (dna3 + 1) / 2; dna_sum = dna0 + dna1 + dna2 + dna3; }
			const double rec = 1.0 / dna_sum;
			const uint32_t x = lane == 0 ? dna0 : lane == 1 ? dna1 : lane == 2 ? dna2 : dna3;
			const double lg = x ? -glibc_log2::log2((double)x * rec) : 0.0;
			dl0 = __shfl(lg, 0); dl1 = __shfl(lg, 1); dl2 = __shfl(lg, 2); dl3 = __shfl(lg, 3);
		}
		for (uint64_t e0 = ev_off[r]; e0 < ev_off[r + 1]; e0 += 64)
		{
			const uint32_t cnt = (uint32_t)(ev_off[r + 1] - e0 < 64 ? ev_off[r + 1] - e0 : 64);
			__syncthreads();
			if (lane < cnt)
			{
				const uint32_t ev = events[e0 + lane];
				ev_id[lane] = ev;
				recs[lane] = T.lv[ev >> 28].pend[ev & 0x0fffffffu];
			}
			__syncthreads();
			for (uint32_t k = 0; k < cnt; ++k)
			{	// EncodeWithEditScript (utils.h:1060-1130)
				const PendRec& p = recs[k];
				const uint32_t rd_l = lane < 12 ? p.rd[lane] : 0u;
				uint32_t rd_sum = rd_l;
				for (int o = 8; o; o >>= 1) rd_sum += __shfl_xor(rd_sum, o);              // lanes 0..15 (12..15 hold 0)
				rd_sum = __shfl(rd_sum, 0);
				const uint32_t loc_l = es_l + rd_l, loc_sum = es_sum + rd_sum;
				const bool dec_resc = dec_sum + 1 > MX;
				uint32_t x = loc_l; double rec = 1.0 / loc_sum;
				if (lane >= 12 && lane < 16)
				{	// decision logarithms after this event: lanes 12, 13 if the edit script wins, 14, 15 if the literal wins
					x = lane == 12 ? dec0 + 1 : lane == 13 ? dec1 : lane == 14 ? dec0 : dec1 + 1;
					rec = 1.0 / (dec_sum + 1);
				}
				const double lg = x ? -glibc_log2::log2((double)x * rec) : 0.0;
				const double term = (double)rd_l * lg;
				double es_cost = dcl0;
#pragma unroll
				for (int i = 0; i < 12; ++i) es_cost += __shfl(term, i);
				es_cost = lens_add(es_cost, p.lens);
				double plain_cost = dcl1;
				plain_cost += p.pl[0] * dl0; plain_cost += p.pl[1] * dl1; plain_cost += p.pl[2] * dl2; plain_cost += p.pl[3] * dl3;
				plain_cost += bitlen32(p.ref_len) + 1;
				const bool choose_plain = plain_cost < es_cost;
				if (choose_plain) ++dec1;
				else
				{
					++dec0; es_l = loc_l; es_sum = loc_sum;
					while (es_sum > MX)
					{
						es_l = (es_l + 1) / 2;
						uint32_t sm = lane < 12 ? es_l : 0u;
						for (int o = 8; o; o >>= 1) sm += __shfl_xor(sm, o);
						es_sum = __shfl(sm, 0);
					}
				}
				++dec_sum;
				if (!dec_resc) { dcl0 = __shfl(lg, choose_plain ? 14 : 12); dcl1 = __shfl(lg, choose_plain ? 15 : 13); }
				else
				{
					while (dec_sum > MX) { dec0 = (dec0 + 1) / 2; dec1 = (dec1 + 1) / 2; dec_sum = dec0 + dec1; }
					const double rc = 1.0 / dec_sum;
					dcl0 = dec0 ? -glibc_log2::log2((double)dec0 * rc) : 0.0; dcl1 = dec1 ? -glibc_log2::log2((double)dec1 * rc) : 0.0;
				}
				if (lane == 0) { const uint32_t ev = ev_id[k]; T.lv[ev >> 28].dec[ev & 0x0fffffffu] = choose_plain ? 0 : 1; }
			}
		}
	}
}
// Tuple emission: one wave per read over the run-length monoid of its fragments (emit_wave.hpp; k_emit_count_wave sizes and tuple counts,
// k_emit_write_wave the bytes), k_emit_plain for reads stored plain (one wave per read, one lane per base).  Rounds 1-2 walked a read's frame
// tree with one lane (emit_read, encode_core.hpp: 12.6 s per pass against 2.1; it stays as the sequential statement the host debugging
// build replays, tests/tools/encode_host.hip).
__global__ __launch_bounds__(256) void k_emit_count_wave(ArenaV A, TreeV T, uint32_t n_reads, const uint32_t* __restrict__ data, uint32_t* __restrict__ sizes, uint32_t* __restrict__ ntuples)
{
	const uint32_t r = blockIdx.x * 4 + (threadIdx.x >> 6);
	if (r >= n_reads) return;
	if (T.frame_of_read[r] == 0xffffffffu) { if ((threadIdx.x & 63) == 0) { sizes[r] = A.lens[r] + 1; ntuples[r] = A.lens[r] + 1; } return; }   // a start tuple and one tuple per base
	emit_read_wave<false>(A, T, r, data, sizes, ntuples, nullptr, nullptr);
}
__global__ __launch_bounds__(256) void k_emit_write_wave(ArenaV A, TreeV T, uint32_t n_reads, const uint32_t* __restrict__ data, const uint64_t* __restrict__ es_off, uint8_t* __restrict__ out)
{
	const uint32_t r = blockIdx.x * 4 + (threadIdx.x >> 6);
	if (r >= n_reads || T.frame_of_read[r] == 0xffffffffu) return;
	emit_read_wave<true>(A, T, r, data, nullptr, nullptr, es_off, out);
}
__global__ __launch_bounds__(256) void k_emit_plain(ArenaV A, const uint32_t* __restrict__ inv, const uint8_t* __restrict__ has_n, const uint32_t* __restrict__ frame_of_read, uint32_t n_reads,
                                                   const uint64_t* __restrict__ es_off, uint8_t* __restrict__ out)
{	// AddPlainRead / AddPlainReadWithN (encoder.cpp:663-681): a start tuple, then one tuple per base
	const uint32_t r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
	if (r >= n_reads || frame_of_read[r] != 0xffffffffu) return;
	const uint32_t len = A.lens[r]; const uint64_t wb = A.word_off[r];
	uint8_t* o = out + es_off[r];
	if (lane == 0) o[0] = (uint8_t)((has_n[r] ? 11 : 9) << 4);
	for (uint32_t i = lane; i < len; i += 64)
	{
		const uint64_t pw = A.packed[wb + (i >> 5)]; const uint32_t iw = inv[wb + (i >> 5)];
		const bool isn = (iw >> (31 - (i & 31))) & 1u;
		o[1 + i] = (uint8_t)((8u << 4) + (isn ? 4u : (uint32_t)(pw >> (62 - 2 * (i & 31))) & 3u));
	}
}

struct LevelBufs {
	DevBuf<FrameRec> frames; DevBuf<CandEnt> cands; DevBuf<GapRec> gaps; DevBuf<char> es; DevBuf<PendRec> pend; DevBuf<uint8_t> dec; DevBuf<GapSum> sums;
	uint32_t n_frames = 0, n_gaps = 0; uint64_t n_cands = 0;
	LevelV view() { return LevelV{ frames.p, cands.p, gaps.p, es.p, pend.p, dec.p, n_frames, n_gaps, sums.p }; }
};
} // namespace
#include "encode_diag.hpp"

// ---- the host driver: what a call knows, what a level knows, the steps of a level ---------------------------------------------------
namespace {
// Every environment switch of this file, read once at the entry of cl_encode_reads: per call, so a tool may set one between two calls
struct EncKnobs {
	uint32_t small_per_cu, quad_waves;   // tuning: blocks of k_align_small per CU (15 - 25 KB of LDS each), waves of k_align_quad_rows at most (18.5 KB each)
	uint32_t wave_debug_stage;           // handed to k_align_wave
	uint32_t tail_row_limit;             // k_gap_tail: scripts up to this many symbols are taken by a row of 16 lanes, longer ones by a wave
	bool no_team_align;                  // the giant gaps go to the wave kernel (tools/giant_check.py's comparison)
	bool gap_debug, gap_shapes, quad_profile, wave_profile, wave_heartbeat;   // the diagnostics of encode_diag.hpp
	static EncKnobs read()
	{
		auto num = [](const char* name, int dflt, int least) { const char* e = getenv(name); return (uint32_t)(e ? std::max(least, atoi(e)) : dflt); };
		auto on = [](const char* name) { return getenv(name) != nullptr; };
		return EncKnobs{ num("COLORD_HIP_SMALL_PER_CU", 4, 1), num("COLORD_HIP_QUAD_WAVES", 2048, 64), num("COLORD_HIP_WAVE_DEBUG_STAGE", 0, INT_MIN),
			num("COLORD_HIP_TAIL_ROW_LIMIT", (int)SUM_LIMIT, 0), on("COLORD_HIP_NO_TEAM_ALIGN"),
			on("COLORD_HIP_GAP_DEBUG"), on("COLORD_HIP_GAP_SHAPES"), on("COLORD_HIP_QUAD_PROFILE"), on("COLORD_HIP_WAVE_PROFILE"), on("COLORD_HIP_WAVE_HEARTBEAT") };
	}
};
// the constants of one call.  st: the context's main stream; n_cu: the device's CUs (cl_ctx_create); err: device word, bit 2 = inconsistent anchors
struct EncCall { cl_ctx* ctx; hipStream_t st; ArenaV A, R; AnchorsV AV; EncCfg cfg; const uint8_t* has_n; uint32_t nr, n_cu; uint32_t* err; EncKnobs knobs; };

// The temporaries of one level that more than one step uses.  All of it lives to the end of the level's loop body: kernels of the main
// stream still read these buffers when the step that launched them returns, and the side streams read ids.  The buffers go back to the
// device pool, which the encode lanes share, in the reverse order of their declaration (profiles/encode_driver_ab.txt: keep that order).
struct LevelWork {
	DevBuf<uint32_t> first, capw, pflag, keys, ids; DevBuf<uint64_t> es_off; DevBuf<uint32_t> bounds;   // gaps: first of a frame; script capacity, "pending" flag (scanned), sort key, id by key; script offset; hb on the device
	uint64_t ng = 0, es_total = 0, n_pend = 0;
	LevelV V;                                          // the level's view, taken before L.sums exists (the kernels that need the sums get them as an argument)
	uint32_t hb[N_CLASSES + 3] = { 0 };                // class c is ids[hb[c] .. hb[c + 1]); [N_CLASSES + 1], [+ 2]: the giants' summed and largest script capacity
	unsigned long long h_cb[2 * N_CLASSES] = { 0 };    // bytes, then DP cells, per class (timing contexts only: 0 otherwise)
	uint32_t count(uint32_t cls) const { return hb[cls + 1] - hb[cls]; }
	const uint32_t* list(uint32_t cls) const { return ids.p + hb[cls]; }
	double bytes(uint32_t cls) const { return 1.25 * (double)h_cb[cls]; }   // 2-bit symbols in, a script byte per symbol out
	double cells(uint32_t cls) const { return (double)h_cb[N_CLASSES + cls]; }
};
// ... and those of its decisions and children (declared after the aligners' objects): spawn flag (scanned), its candidates, the list of the gaps whose scripts are beyond the row limit, candidate offset
struct SpawnWork { DevBuf<uint32_t> sflag, sncand, over_list; DevBuf<uint64_t> cbase; };

// Joins a side stream on every way out of its scope.  As the LAST member of an object it is destroyed FIRST: the object's buffers
// outlive the kernels of the stream that use them, also when a step returns early with an error.
struct StreamJoin {
	hipStream_t s = nullptr;
	~StreamJoin() { if (s) (void)hipStreamSynchronize(s); }
	// waits for the stream (a host wait) and returns the second word of its aligner's two-word counter: the gaps it hands back
	cl_status redo_count(cl_ctx* ctx, const unsigned int* cnt, uint32_t& n_redo)
	{
		unsigned int hc[2];
		HIP_TRY(ctx, hipMemcpyAsync(hc, cnt, 8, hipMemcpyDeviceToHost, s));
		HIP_TRY(ctx, hipStreamSynchronize(s));
		s = nullptr;
		n_redo = hc[1];
		return CL_OK;
	}
};

using Levels = std::vector<std::unique_ptr<LevelBufs>>;
// level 0: one frame per read that has candidates.  Host waits (main stream): two scan totals, then the frames (flag / ncand / cbase go)
cl_status level0_frames(const EncCall& E, uint32_t* frame_of_read, Levels& levels)
{
	cl_ctx* ctx = E.ctx; const uint32_t nr = E.nr;
	auto L = std::make_unique<LevelBufs>();
	DevBuf<uint32_t> flag, ncand; DEV_ALLOC(ctx, flag, (uint64_t)nr + 1); DEV_ALLOC(ctx, ncand, (uint64_t)nr + 1);
	DevBuf<uint64_t> cbase; DEV_ALLOC(ctx, cbase, (uint64_t)nr + 1);
	LAUNCH(ctx, k_read_flags, grid_for(nr, 256), 256, E.AV.n_cands, E.has_n, nr, flag.p, ncand.p);
	uint64_t nf = 0;
	CL_TRY(dev_exclusive_scan_u64(ctx, ncand.p, cbase.p, nr, &L->n_cands));
	CL_TRY(dev_exclusive_scan_u32(ctx, flag.p, nr, &nf));
	L->n_frames = (uint32_t)nf;
	DEV_ALLOC(ctx, L->frames, nf + 1); DEV_ALLOC(ctx, L->cands, L->n_cands + 1);
	LAUNCH(ctx, k_frames_level0, grid_for(nr, 256), 256, E.A, E.AV, E.cfg.c, E.has_n, nr, (const uint32_t*)flag.p, (const uint64_t*)cbase.p, L->frames.p, L->cands.p, frame_of_read);
	HIP_TRY(ctx, hipGetLastError());
	HIP_TRY(ctx, hipStreamSynchronize(E.st));
	levels.push_back(std::move(L));
	return CL_OK;
}

// the gaps of a level: counts -> scan -> geometry -> scans -> offsets, and the level's buffers as their sizes become known.
// Host waits (main stream): the three scan totals — gaps, script symbols, pending slots — each of which sizes the next allocation
cl_status level_gaps(const EncCall& E, LevelBufs& L, LevelWork& W)
{
	cl_ctx* ctx = E.ctx;
	DEV_ALLOC(ctx, W.first, (uint64_t)L.n_frames + 1);
	LAUNCH(ctx, k_frame_gap_counts, grid_for(L.n_frames, 256), 256, (const FrameRec*)L.frames.p, (const CandEnt*)L.cands.p, L.n_frames, W.first.p);
	CL_TRY(dev_exclusive_scan_u32(ctx, W.first.p, L.n_frames, &W.ng));
	const uint64_t ng = W.ng;
	if (ng >= (1ull << 32)) return cl_fail(ctx, CL_E_UNSUPPORTED, "cl_encode_reads: more than 2^32 gaps in one call");
	L.n_gaps = (uint32_t)ng;
	LAUNCH(ctx, k_frame_first_gaps, grid_for(L.n_frames, 256), 256, L.frames.p, (const uint32_t*)W.first.p, L.n_frames, L.n_gaps);
	DEV_ALLOC(ctx, L.gaps, ng + 1);
	DEV_ALLOC(ctx, W.capw, ng + 1); DEV_ALLOC(ctx, W.pflag, ng + 1); DEV_ALLOC(ctx, W.keys, ng + 1); DEV_ALLOC(ctx, W.ids, ng + 1);
	LAUNCH(ctx, k_gap_geometry, grid_for(ng, 256), 256, L.view(), E.R, E.AV.data, E.cfg.min_part_alt, (const uint32_t*)W.first.p, W.capw.p, W.pflag.p, W.keys.p, W.ids.p, E.err);
	DEV_ALLOC(ctx, W.es_off, ng + 1);
	CL_TRY(dev_exclusive_scan_u64(ctx, W.capw.p, W.es_off.p, ng, &W.es_total));
	CL_TRY(dev_exclusive_scan_u32(ctx, W.pflag.p, ng, &W.n_pend));
	LAUNCH(ctx, k_gap_offsets, grid_for(ng, 256), 256, L.gaps.p, (const uint64_t*)W.es_off.p, L.n_gaps);
	DEV_ALLOC(ctx, L.es, W.es_total + 16); DEV_ALLOC(ctx, L.pend, W.n_pend + 1); DEV_ALLOC(ctx, L.dec, W.n_pend + 1);
	W.V = L.view();
	return CL_OK;
}

// size classes: the gaps sorted by class and size; the class bounds hb (on a timing context each class's bytes and cells, h_cb, too) on the
// host.  Host waits (main stream): the end of the sort (its temporaries go), then hb / h_cb: every aligner launch is sized by them
cl_status level_size_classes(const EncCall& E, LevelBufs& L, LevelWork& W)
{
	cl_ctx* ctx = E.ctx; const uint64_t ng = W.ng;
	CL_TRY(dev_sort_keys32_pairs(ctx, W.keys.p, W.ids.p, ng, 0, KEY_BITS));
	DEV_ALLOC(ctx, W.bounds, N_CLASSES + 3);
	HIP_TRY(ctx, hipMemsetAsync(W.bounds.p + N_CLASSES + 1, 0, 8, E.st));
	LAUNCH(ctx, k_class_bounds, grid_for(ng + 1, 256), 256, (const uint32_t*)W.keys.p, (const uint32_t*)W.ids.p, (const uint32_t*)W.capw.p, L.n_gaps, W.bounds.p);
	HIP_TRY(ctx, hipMemcpyAsync(W.hb, W.bounds.p, 4 * (N_CLASSES + 3), hipMemcpyDeviceToHost, E.st));
	if (ctx->timing)
	{
		DevBuf<unsigned long long> cb; DEV_ALLOC(ctx, cb, 2 * N_CLASSES);
		HIP_TRY(ctx, hipMemsetAsync(cb.p, 0, 16 * N_CLASSES, E.st));
		LAUNCH(ctx, k_class_bytes, grid_for(ng, 256), 256, (const uint32_t*)W.keys.p, (const uint32_t*)W.ids.p, (const uint32_t*)W.capw.p, (const GapRec*)L.gaps.p, L.n_gaps, cb.p);
		HIP_TRY(ctx, hipMemcpyAsync(W.h_cb, cb.p, 16 * N_CLASSES, hipMemcpyDeviceToHost, E.st));
	}
	HIP_TRY(ctx, hipStreamSynchronize(E.st));
	return CL_OK;
}

// classes 1 - 4 (rows <= 64 NB, columns <= 256), one lane per gap with its state in LDS, on the stream `side`: next to the large ones on
// the main stream (one wave per SIMD here, five waves per SIMD on a bump pool in HBM there: they share the machine well)
struct SmallAligner {
	DevBuf<uint64_t> hist;
	StreamJoin join;
	cl_status launch(const EncCall& E, LevelBufs& L, const LevelWork& W)
	{
		cl_ctx* ctx = E.ctx;
		HIP_TRY(ctx, cl_side_stream(ctx, ctx->side));
		join.s = ctx->side;
		const uint32_t cap_blocks = E.n_cu * E.knobs.small_per_cu;
		uint32_t max_blocks = 1;
		for (int nb = 1; nb <= 4; ++nb) max_blocks = std::max(max_blocks, std::min<uint32_t>(grid_for(W.count(nb), 64), cap_blocks));
		DEV_ALLOC(ctx, hist, (uint64_t)max_blocks * 256 * 4 * 2 * 64);
		LaunchOn on(ctx, ctx->side);                                          // (launches + timing events on the side stream)
		hipError_t le = hipSuccess;
		for (int nb = 1; nb <= 4; ++nb)
		{
			const uint32_t n_list = W.count(nb);
			if (!n_list) continue;
			const uint32_t blocks = std::min<uint32_t>(grid_for(n_list, 64), cap_blocks);
			const uint32_t lds = (12 * nb + 48) * 64 * 4;                       // LdsMem<nb>: QW + TW + EW words per lane
			const double bytes = W.bytes(nb); const uint32_t* list = W.list(nb);
			ctx->next_cells = W.cells(nb);
			switch (nb)
			{
			case 1: LAUNCHB_SHM(ctx, bytes, (k_align_small<1>), blocks, 64, lds, list, n_list, L.gaps.p, L.es.p, E.A, E.R, hist.p); break;
			case 2: LAUNCHB_SHM(ctx, bytes, (k_align_small<2>), blocks, 64, lds, list, n_list, L.gaps.p, L.es.p, E.A, E.R, hist.p); break;
			case 3: LAUNCHB_SHM(ctx, bytes, (k_align_small<3>), blocks, 64, lds, list, n_list, L.gaps.p, L.es.p, E.A, E.R, hist.p); break;
			default: LAUNCHB_SHM(ctx, bytes, (k_align_small<4>), blocks, 64, lds, list, n_list, L.gaps.p, L.es.p, E.A, E.R, hist.p); break;
			}
			if (le == hipSuccess) le = hipGetLastError();
		}
		HIP_TRY(ctx, le);
		return CL_OK;
	}
	// Host wait (side).  (The guard stays armed: it joins the idle stream once more at the end of the level.)
	cl_status wait(cl_ctx* ctx) { HIP_TRY(ctx, hipStreamSynchronize(ctx->side)); return CL_OK; }
};

// class 5 (up to 16 row blocks): four gaps per wave on the stream `side2` — a throughput kernel next to the wave-per-gap kernel, whose
// launches last as long as their single slowest gap (measured: launch 61.5 ms, slowest gap 61.4 ms) and leave the machine idle
// meanwhile.  The few gaps whose distance is beyond the band or whose buffers do not fit a wave's pool come back in `redo`.
struct QuadAligner {
	DevBuf<uint32_t> redo; DevBuf<uint8_t> scratch; DevBuf<unsigned int> cnt;
	StreamJoin join;                                                         // armed from the first command on side2 to finish()
	cl_status launch(const EncCall& E, uint32_t lv, LevelBufs& L, const LevelWork& W)
	{
		cl_ctx* ctx = E.ctx;
		const uint32_t n_list = W.count(5);
		if (!n_list) return CL_OK;
		// 2.25 MB a wave: four banded histories of at most 512 KB; 2048 waves (4096 were no faster beside the other streams)
		const uint64_t per_wave = 9ull << 18;
		const uint32_t waves = std::min<uint32_t>((n_list + 3) / 4, E.knobs.quad_waves);
		DEV_ALLOC(ctx, scratch, per_wave * waves);
		DEV_ALLOC(ctx, cnt, 2);
		DEV_ALLOC(ctx, redo, (uint64_t)n_list + 1);
		HIP_TRY(ctx, cl_side_stream(ctx, ctx->side2));
		join.s = ctx->side2;
		HIP_TRY(ctx, hipMemsetAsync(cnt.p, 0, 8, ctx->side2));
		LaunchOn on(ctx, ctx->side2);                                         // (launch + timing events on the third stream)
		DevBuf<unsigned long long> qp;                                        // (COLORD_HIP_QUAD_PROFILE: the phases of the row kernel; waits for the launch)
		if (E.knobs.quad_profile) { DEV_ALLOC(ctx, qp, 16); HIP_TRY(ctx, hipMemsetAsync(qp.p, 0, 128, ctx->side2)); }
		ctx->next_cells = W.cells(5);
		if (qp.p) LAUNCHB(ctx, W.bytes(5), k_align_quad_rows<true>, waves, 64, W.list(5), n_list, L.gaps.p, L.es.p, E.A, E.R, scratch.p, per_wave, cnt.p, redo.p, cnt.p + 1, qp.p);
		else LAUNCHB(ctx, W.bytes(5), k_align_quad_rows<false>, waves, 64, W.list(5), n_list, L.gaps.p, L.es.p, E.A, E.R, scratch.p, per_wave, cnt.p, redo.p, cnt.p + 1, (unsigned long long*)nullptr);
		if (qp.p) CL_TRY(diag::quad_profile(ctx, ctx->side2, qp.p, lv, n_list, waves));
		HIP_TRY(ctx, hipGetLastError());
		return CL_OK;
	}
	// Host wait (side2), if the level has class-5 gaps: how many of them the row kernel hands back
	cl_status finish(cl_ctx* ctx, uint32_t& n_redo) { n_redo = 0; return join.s ? join.redo_count(ctx, cnt.p, n_redo) : CL_OK; }
};

// class 7, the giant gaps: many waves each (align_giant.hpp), on the stream `side3` from the start of the level, next to everything else
struct GiantAligner {
	DevBuf<uint32_t> redo; DevBuf<uint8_t> mem, heap, scratch; DevBuf<unsigned int> cnt;
	StreamJoin join;                                                         // armed from the first command on side3 to finish()
	bool running() const { return join.s != nullptr; }
	cl_status launch(const EncCall& E, LevelBufs& L, const LevelWork& W)
	{
		cl_ctx* ctx = E.ctx;
		const uint32_t n_list = W.count(7);
		if (!n_list || E.knobs.no_team_align) return CL_OK;
		const uint64_t sum_cap = (uint64_t)W.hb[N_CLASSES + 1] * 256, max_cap = W.hb[N_CLASSES + 2];
		// sequences (4 copies), operations, sparse operations: 6 x (reference + read symbols) per gap; the last columns of a Hirschberg
		// level: 8 bytes per row and level, the hand-over pairs 2 bits per column and tile
		const uint64_t heap_bytes = std::min<uint64_t>(6ull << 30, (64ull << 20) + 100 * sum_cap + (uint64_t)n_list * 4096);
		uint32_t phases = 2; for (uint64_t c = max_cap; c > 8 && phases < gt::MAX_PHASES; c >>= 1) ++phases;     // the columns halve per level; below ~16 everything is a leaf
		auto al = [](uint64_t x) { return (x + 255) & ~255ull; };
		const uint64_t o_ctl = 0, o_flags = al(sizeof(gt::Ctl)), o_nodes = o_flags + al(4ull * gt::FLAG_CAP), o_sweeps = o_nodes + 2 * al(sizeof(gt::Node) * gt::NODE_CAP),
			o_jobs = o_sweeps + 2 * al(sizeof(gt::Sweep) * 2 * gt::NODE_CAP), o_leaves = o_jobs + 2 * al(sizeof(gt::Job) * gt::JOB_CAP), o_giants = o_leaves + al(sizeof(gt::Leaf) * gt::LEAF_CAP),
			o_end = o_giants + al(sizeof(gt::Giant) * n_list);
		DEV_ALLOC(ctx, mem, o_end); DEV_ALLOC(ctx, heap, heap_bytes);
		const uint32_t leaf_waves = 256; const uint64_t per_wave = 3ull << 20;     // a leaf's history is < 1 MiB twice over, + the reversed operations
		const uint32_t fin_waves = std::min<uint32_t>(n_list, 64); const uint64_t fin_per_wave = (per_wave * leaf_waves) / 64;   // 12 MB: the canonicalisation's 9 bytes per script symbol
		DEV_ALLOC(ctx, scratch, per_wave * leaf_waves);
		DEV_ALLOC(ctx, cnt, 2);
		DEV_ALLOC(ctx, redo, (uint64_t)n_list + 1);
		HIP_TRY(ctx, cl_side_stream(ctx, ctx->side3));
		join.s = ctx->side3;
		HIP_TRY(ctx, hipMemsetAsync(cnt.p, 0, 8, ctx->side3));
		HIP_TRY(ctx, hipMemsetAsync(mem.p, 0, o_nodes, ctx->side3));              // the control block and the progress words
		gt::View V; V.ctl = (gt::Ctl*)(mem.p + o_ctl); V.heap = heap.p; V.heap_bytes = heap_bytes; V.flags = (uint32_t*)(mem.p + o_flags);
		for (int i = 0; i < 2; ++i) { V.nodes[i] = (gt::Node*)(mem.p + o_nodes + i * al(sizeof(gt::Node) * gt::NODE_CAP)); V.sweeps[i] = (gt::Sweep*)(mem.p + o_sweeps + i * al(sizeof(gt::Sweep) * 2 * gt::NODE_CAP));
			V.jobs[i] = (gt::Job*)(mem.p + o_jobs + i * al(sizeof(gt::Job) * gt::JOB_CAP)); }
		V.leaves = (gt::Leaf*)(mem.p + o_leaves); V.giants = (gt::Giant*)(mem.p + o_giants); V.n_giants = n_list; V.n_phases = phases;
		LaunchOn on(ctx, ctx->side3);
		ctx->next_cells = W.cells(7);                                          // (booked on the staging launch: the class as a whole is what the report adds up)
		LAUNCHB(ctx, W.bytes(7), k_giant_stage, n_list, 256, V, W.list(7), (const GapRec*)L.gaps.p, E.A, E.R);
		for (uint32_t ph = 0; ph < phases; ++ph) LAUNCH(ctx, k_giant_level, 1024, 64, V, ph);
		LAUNCH(ctx, k_giant_leaves, leaf_waves, 64, V, scratch.p, per_wave);
		LAUNCH(ctx, k_giant_finish, fin_waves, 64, V, L.gaps.p, L.es.p, scratch.p, fin_per_wave, cnt.p, redo.p, cnt.p + 1);
		HIP_TRY(ctx, hipGetLastError());
		return CL_OK;
	}
	// Host wait (side3), if running(): how many giants the tile jobs hand back
	cl_status finish(cl_ctx* ctx, uint32_t& n_redo) { return join.redo_count(ctx, cnt.p, n_redo); }
};

// class 6 and what the other aligners hand back: a wave per gap (k_align_wave) on the main stream, in rounds of growing pools.  3 MB a
// wave: since the sweeps stop at the saturation row, sequences + operations + history of nearly every gap fit (a read flank of 200 kb:
// 1.6 MB); the few others come back in the next round (x 8).  alg_bytes / cells are booked on round 0's launch.  level_class: the list
// is the level's wave class, not a redo list.  Host waits (main stream), per round: its redo count; with gaps left, the copy of its redo list
cl_status wave_rounds(const EncCall& E, uint32_t lv, LevelBufs& L, const LevelWork& W, const uint32_t* list, uint32_t n_list, double alg_bytes, double cells, bool level_class)
{
	cl_ctx* ctx = E.ctx; hipStream_t st = E.st;
	if (n_list && E.knobs.gap_debug && level_class) CL_TRY(diag::wave_class_shapes(ctx, st, lv, L, W.hb, list, n_list));
	DevBuf<uint32_t> todo, redo; DEV_ALLOC(ctx, todo, (uint64_t)n_list + 1); DEV_ALLOC(ctx, redo, (uint64_t)n_list + 1);
	DevBuf<unsigned int> cnt; DEV_ALLOC(ctx, cnt, 2);
	uint64_t per_wave = 3ull << 20; uint32_t max_waves = 2048;
	DevBuf<unsigned long long> prof;
	if (E.knobs.wave_profile) { DEV_ALLOC(ctx, prof, 16); HIP_TRY(ctx, hipMemsetAsync(prof.p, 0, 128, st)); }
	uint32_t* hbt_dev = nullptr;
	if (n_list && E.knobs.wave_heartbeat) CL_TRY(diag::wave_heartbeat(ctx, &hbt_dev));
	for (int round = 0; n_list; ++round)
	{
		if (round == 5) return cl_fail(ctx, CL_E_NOMEM, "cl_encode_reads: lane pool exhausted (" + std::to_string(n_list) + " gaps left)");
		const uint32_t waves = std::min<uint32_t>(n_list, max_waves);
		DevBuf<uint8_t> scratch; DEV_ALLOC(ctx, scratch, per_wave * waves);
		HIP_TRY(ctx, hipMemsetAsync(cnt.p, 0, 8, st));
		const auto t_launch = std::chrono::steady_clock::now();               // (for the profile's line)
		if (round == 0) ctx->next_cells = cells;
		LAUNCHB(ctx, round == 0 ? alg_bytes : 0.0, k_align_wave, waves, 64, list, n_list, L.gaps.p, L.es.p, E.A, E.R, scratch.p, per_wave, cnt.p, redo.p, cnt.p + 1,
			E.knobs.wave_debug_stage, hbt_dev, prof.p);
		if (prof.p) CL_TRY(diag::wave_profile(ctx, st, prof.p, lv, n_list, waves, t_launch));
		HIP_TRY(ctx, hipGetLastError());
		unsigned int hc[2];
		HIP_TRY(ctx, hipMemcpyAsync(hc, cnt.p, 8, hipMemcpyDeviceToHost, st));
		HIP_TRY(ctx, hipStreamSynchronize(st));
		n_list = hc[1];
		if (n_list)
		{
			HIP_TRY(ctx, hipMemcpyAsync(todo.p, redo.p, (uint64_t)n_list * 4, hipMemcpyDeviceToDevice, st));
			HIP_TRY(ctx, hipStreamSynchronize(st));
			list = todo.p;
			++ctx->gap_paths[10];                                               // a further round with larger pools
		}
		per_wave *= 8; max_waves = std::max<uint32_t>(max_waves / 8, 64);
	}
	return CL_OK;
}

// statistics / decisions of the level's gaps, and which of them get a child frame (k_spawn_mark refuses beyond max_rec: those gaps
// become literals).  No host wait
cl_status level_decisions(const EncCall& E, LevelBufs& L, const LevelWork& W, SpawnWork& S)
{
	cl_ctx* ctx = E.ctx; const uint64_t ng = W.ng;
	DEV_ALLOC(ctx, S.sflag, ng + 1); DEV_ALLOC(ctx, S.sncand, ng + 1);
	DEV_ALLOC(ctx, L.sums, ng + 1);
	DEV_ALLOC(ctx, S.over_list, ng + 2);                                       // ids of the gaps left to the whole-wave kernels, their number in the last word
	unsigned int* n_over = (unsigned int*)(S.over_list.p + ng + 1);
	HIP_TRY(ctx, hipMemsetAsync(n_over, 0, 4, E.st));
	// algorithmic bytes: the scripts (about half their capacity of reference + read symbols) and the read's 2-bit bases under them, a gap
	// record read and written, id, pending index, spawn flag and summary per gap, a pending record per short gap
	const double tail_bytes = 0.625 * (double)W.es_total + (double)ng * (2 * sizeof(GapRec) + sizeof(GapSum) + 12) + (double)W.n_pend * sizeof(PendRec);
	LAUNCHB(ctx, tail_bytes, k_gap_tail, grid_for(ng * 16, 256), 256, W.V, E.A, E.cfg, (const uint32_t*)W.ids.p, (const uint32_t*)W.pflag.p, L.sums.p, S.sflag.p,
		E.knobs.tail_row_limit, S.over_list.p, n_over);
	LAUNCH(ctx, k_gap_stats_long, 1024, 256, W.V, E.A, E.cfg, (const uint32_t*)W.pflag.p, (const uint32_t*)S.over_list.p, (const unsigned int*)n_over, S.sflag.p);
	LAUNCH(ctx, k_gap_sums_long, 1024, 256, W.V, L.sums.p, (const uint32_t*)S.over_list.p, (const unsigned int*)n_over);
	LAUNCH(ctx, k_spawn_mark, grid_for(ng, 64), 64, W.V, E.AV.data, E.cfg, S.sflag.p, S.sncand.p);
	HIP_TRY(ctx, hipGetLastError());
	return CL_OK;
}

// the next level's frames and candidates, added to `levels` — unless no gap spawned a frame: the level loop ends there.  Host waits (main
// stream): two scan totals — candidates, frames — that size the child level, then the end of the level (its temporaries go)
cl_status level_spawn(const EncCall& E, const LevelWork& W, SpawnWork& S, Levels& levels)
{
	cl_ctx* ctx = E.ctx; const uint64_t ng = W.ng;
	auto N = std::make_unique<LevelBufs>();
	DEV_ALLOC(ctx, S.cbase, ng + 1);
	uint64_t nf = 0;
	CL_TRY(dev_exclusive_scan_u64(ctx, S.sncand.p, S.cbase.p, ng, &N->n_cands));
	CL_TRY(dev_exclusive_scan_u32(ctx, S.sflag.p, ng, &nf));
	N->n_frames = (uint32_t)nf;
	if (!nf) return CL_OK;
	DEV_ALLOC(ctx, N->frames, nf + 1); DEV_ALLOC(ctx, N->cands, N->n_cands + 1);
	LAUNCH(ctx, k_spawn_fill, grid_for(ng, 64), 64, W.V, E.AV.data, E.cfg, (const uint32_t*)S.sflag.p, (const uint64_t*)S.cbase.p, N->frames.p, N->cands.p);
	HIP_TRY(ctx, hipGetLastError());
	HIP_TRY(ctx, hipStreamSynchronize(E.st));
	levels.push_back(std::move(N));
	return CL_OK;
}

// estimator (per reader pack), then tuples: sizes, offsets, bytes.  Host waits (main stream): the scan totals of the estimator's events
// and of the tuple bytes (checked against the caller's capacity), then the end of the call
cl_status estimate_and_emit(const EncCall& E, const cl_reads* reads, const Levels& levels, const uint32_t* frame_of_read, const uint32_t* h_pack_bounds, uint32_t n_packs,
                            uint8_t* d_es, uint64_t cap, uint64_t* d_es_off, uint32_t* d_es_ntuples, uint64_t* n_out)
{
	cl_ctx* ctx = E.ctx; const uint32_t nr = E.nr;
	TreeV T; memset(&T, 0, sizeof(T));
	for (size_t i = 0; i < levels.size() && i < 10; ++i) T.lv[i] = levels[i]->view();
	T.frame_of_read = frame_of_read;
	DevBuf<uint32_t> base_counts; DEV_ALLOC(ctx, base_counts, 4ull * nr);
	LAUNCHB(ctx, reads->total_bases / 4.0, k_read_base_counts, grid_for((uint64_t)nr * 64, 256), 256, E.A, E.has_n, nr, base_counts.p);
	DevBuf<uint32_t> d_pb; DEV_ALLOC(ctx, d_pb, (uint64_t)n_packs + 1);
	HIP_TRY(ctx, hipMemcpyAsync(d_pb.p, h_pack_bounds, ((uint64_t)n_packs + 1) * 4, hipMemcpyHostToDevice, E.st));
	DevBuf<uint32_t> ev_cnt; DEV_ALLOC(ctx, ev_cnt, (uint64_t)nr + 1);
	DevBuf<uint64_t> ev_off; DEV_ALLOC(ctx, ev_off, (uint64_t)nr + 1);
	LAUNCH(ctx, k_pend_count, grid_for(nr, 64), 64, T, nr, ev_cnt.p);
	uint64_t n_events = 0;
	CL_TRY(dev_exclusive_scan_u64(ctx, ev_cnt.p, ev_off.p, nr, &n_events));
	DevBuf<uint32_t> events; DEV_ALLOC(ctx, events, n_events + 1);
	LAUNCH(ctx, k_pend_list, grid_for(nr, 64), 64, T, nr, (const uint64_t*)ev_off.p, events.p);
	if (n_packs) LAUNCH(ctx, k_estimator, n_packs, 64, T, (const uint32_t*)d_pb.p, n_packs, (const uint32_t*)reads->lens.p, E.has_n, (const uint32_t*)base_counts.p, (const uint64_t*)ev_off.p, (const uint32_t*)events.p);
	DevBuf<uint32_t> sizes; DEV_ALLOC(ctx, sizes, nr);
	uint64_t total = 0;
	// one wave per read, the lanes over the fragments of a frame (emit_wave.hpp)
	LAUNCHB(ctx, reads->total_bases * 1.25, k_emit_count_wave, grid_for(nr, 4), 256, E.A, T, nr, E.AV.data, sizes.p, d_es_ntuples);
	HIP_TRY(ctx, hipGetLastError());
	CL_TRY(dev_exclusive_scan_u64(ctx, sizes.p, d_es_off, nr, &total));
	*n_out = total;
	if (total > cap || (total && !d_es)) return cl_fail(ctx, CL_E_CAPACITY, "cl_encode_reads: need " + std::to_string(total) + " bytes");
	LAUNCHB(ctx, reads->total_bases * 1.25 + (double)total, k_emit_write_wave, grid_for(nr, 4), 256, E.A, T, nr, E.AV.data, (const uint64_t*)d_es_off, d_es);
	LAUNCH(ctx, k_emit_plain, grid_for(nr, 4), 256, E.A, (const uint32_t*)reads->inv.p, E.has_n, frame_of_read, nr, (const uint64_t*)d_es_off, d_es);
	HIP_TRY(ctx, hipGetLastError());
	HIP_TRY(ctx, hipStreamSynchronize(E.st));
	return CL_OK;
}
} // namespace

// CEncoder::Encode for all reads of the arena (encoder.cpp:1672-1691).  h_pack_bounds: the reader packs (the
// estimator is reset at every pack).  Output: tuple streams (es_t bytes) back to back.
extern "C" cl_status cl_encode_reads(cl_ctx* ctx, const cl_reads* reads, const cl_reads* refs, const cl_anchors* anchors, uint32_t c, uint32_t anchor_len,
                                     uint32_t min_part_alt, uint32_t max_rec, double cost_mult, const uint32_t* h_pack_bounds, uint32_t n_packs,
                                     uint8_t* d_es, uint64_t cap, uint64_t* d_es_off, uint32_t* d_es_ntuples, uint64_t* n_out)
{
	if (!ctx || !reads || !refs || !anchors || !h_pack_bounds || !d_es_off || !d_es_ntuples || !n_out) return cl_fail(ctx, CL_E_INVALID, "cl_encode_reads: null argument");
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	const uint32_t nr = reads->n_reads;
	if (n_packs && (h_pack_bounds[0] != 0 || h_pack_bounds[n_packs] != nr)) return cl_fail(ctx, CL_E_INVALID, "cl_encode_reads: packs must cover the arena");
	if (max_rec > 8 || c > 16) return cl_fail(ctx, CL_E_UNSUPPORTED, "cl_encode_reads: max_rec <= 8 and c <= 16");
	*n_out = 0;
	for (uint64_t& x : ctx->gap_paths) x = 0;
	if (!nr) return CL_OK;

	Levels levels;
	DevBuf<uint32_t> frame_of_read; DEV_ALLOC(ctx, frame_of_read, nr);
	DevBuf<uint32_t> err; DEV_ALLOC(ctx, err, 1);
	HIP_TRY(ctx, hipMemsetAsync(err.p, 0, 4, ctx->stream));
	const EncCall E{ ctx, ctx->stream, ArenaV{ reads->packed.p, reads->word_off.p, reads->lens.p }, ArenaV{ refs->packed.p, refs->word_off.p, refs->lens.p },
		AnchorsV{ cl_anchors_n_cands(anchors), cl_anchors_cands(anchors), cl_anchors_cand_offsets(anchors), cl_anchors_data(anchors) },
		EncCfg{ c, anchor_len, min_part_alt, max_rec, cost_mult }, reads->has_n.p, nr, (uint32_t)std::max(1, ctx->n_cu), err.p, EncKnobs::read() };
	CL_TRY(level0_frames(E, frame_of_read.p, levels));                       // waits (main): 2 scan totals; the frames of level 0
	for (uint32_t lv = 0; lv < levels.size(); ++lv)
	{
		LevelBufs& L = *levels[lv];
		if (!L.n_frames) break;
		LevelWork W;
		SmallAligner small; QuadAligner quad; GiantAligner giant;              // after W: their streams read W.ids, and they are joined before W goes
		SpawnWork S;
		uint32_t n_quad_redo = 0, n_giant_redo = 0;
		CL_TRY(level_gaps(E, L, W));                                           // waits (main): 3 scan totals — gaps, script symbols, pending slots
		CL_TRY(level_size_classes(E, L, W));                                   // waits (main): the sort's end; the class bounds that size every aligner launch
		CL_TRY(small.launch(E, L, W));                                         // classes 1 - 4 on side
		CL_TRY(quad.launch(E, lv, L, W));                                      // class 5 on side2
		CL_TRY(giant.launch(E, L, W));                                         // class 7 on side3
		CL_TRY(wave_rounds(E, lv, L, W, W.list(6), W.count(6), W.bytes(6), W.cells(6), true));   // class 6 on main; waits (main): each round's redo count
		CL_TRY(quad.finish(ctx, n_quad_redo));                                 // waits (side2): class 5 is through; its redo count
		if (n_quad_redo) CL_TRY(wave_rounds(E, lv, L, W, quad.redo.p, n_quad_redo, 0.0, 0.0, false));
		if (giant.running())
		{
			CL_TRY(giant.finish(ctx, n_giant_redo));                             // waits (side3): class 7 is through; its redo count
			if (E.knobs.gap_debug) diag::giant_line(lv, W.hb, n_giant_redo);
		}
		else if (W.count(7)) CL_TRY(wave_rounds(E, lv, L, W, W.list(7), W.count(7), W.bytes(7), 0.0, false));   // (COLORD_HIP_NO_TEAM_ALIGN)
		if (n_giant_redo) CL_TRY(wave_rounds(E, lv, L, W, giant.redo.p, n_giant_redo, 0.0, 0.0, false));
		for (uint32_t cls = 0; cls < N_CLASSES; ++cls) ctx->gap_paths[cls] += W.count(cls);
		ctx->gap_paths[8] += n_quad_redo; ctx->gap_paths[9] += n_giant_redo;
		if (E.knobs.gap_debug) diag::level_line(ctx, lv, W.hb, n_quad_redo, n_giant_redo);
		CL_TRY(small.wait(ctx));                                               // waits (side): classes 1 - 4 are through — every script of the level is written
		if (E.knobs.gap_shapes) CL_TRY(diag::gap_shapes(ctx, lv, L, W.es_total));
		CL_TRY(level_decisions(E, L, W, S));
		if (lv >= max_rec || lv + 1 >= 10) { HIP_TRY(ctx, hipStreamSynchronize(E.st)); break; }   // waits (main): the last level's decisions, before its temporaries go
		CL_TRY(level_spawn(E, W, S, levels));                                  // waits (main): 2 scan totals — candidates, frames; the end of the level
	}
	uint32_t herr = 0;
	HIP_TRY(ctx, hipMemcpyAsync(&herr, err.p, 4, hipMemcpyDeviceToHost, E.st));
	HIP_TRY(ctx, hipStreamSynchronize(E.st));                                // waits (main): the error word of all levels
	if (herr) return cl_fail(ctx, CL_E_INVALID, "cl_encode_reads: inconsistent anchors");
	CL_TRY(estimate_and_emit(E, reads, levels, frame_of_read.p, h_pack_bounds, n_packs, d_es, cap, d_es_off, d_es_ntuples, n_out));   // waits (main): 2 scan totals; the end of the call
	cl_timing_collect(ctx);
	return CL_OK;
}

// The decision logarithm on its own (calc_logs, utils.h:800-810), so that tests can pin it against the host's libm over
// the reachable (count, total) pairs: same translation unit, same flags, same log2 as k_estimator and gap_stats.
namespace {
__global__ void k_estimator_logs(const uint32_t* __restrict__ cnt, const uint32_t* __restrict__ tot, uint64_t n, double* __restrict__ out)
{
	const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n) return;
	const uint32_t x = cnt[i];
	const double rec = 1.0 / tot[i];
	out[i] = x ? -glibc_log2::log2((double)x * rec) : 0.0;
}
} // namespace
extern "C" cl_status cl_estimator_logs(cl_ctx* ctx, const uint32_t* d_count, const uint32_t* d_total, uint64_t n, double* d_out)
{
	if (!ctx || (n && (!d_count || !d_total || !d_out))) return cl_fail(ctx, CL_E_INVALID, "cl_estimator_logs: null argument");
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	if (n) LAUNCH(ctx, k_estimator_logs, grid_for(n, 256), 256, d_count, d_total, n, d_out);
	HIP_TRY(ctx, hipGetLastError());
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	return CL_OK;
}
