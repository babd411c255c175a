// pileup.hip — per-position base counts of a reference-genome run on the device (pileup.hpp): cl_pileup over the tuple
// streams that cl_encode_reads wrote; the host twin's C entry; the pipeline's hook (pileup_chunk) and the compressor's table.
//
// k_pileup_walk walks the streams as es_wave.hpp describes: ONE WAVE PER READ, the stream 64 bytes per window (a byte per lane), the
// tuple starts from three ballots, the window cut into stretches on one reference at alt-id / main-ref; inside a stretch a wave prefix
// sum of the cursor advances gives every tuple its cursor.  Every start lane books its OWN tuple: a del, match or subst lane one
// atomicAdd into its position's counter, an anchor lane two into `diff` (+1 at its first position, -1 behind its last), the lane that
// opens an insertion run one.  Subst lanes alone load a reference base (EsRefs<true>, ref_base).  "The tuple before me is an ins" is the
// ins ballot shifted by a lane — an ins is one byte, so the tuple before starts at the lane before or that lane is payload — and
// across windows one uniform carried bit.  What is uniform per read (insertion runs without a position, whether a genome piece was
// touched) leaves by one 64-bit atomic from lane 0.  Persistent blocks of four waves stride over the reads; no LDS, no barrier.
// k_pileup_tile_sums / k_pileup_fold: a wave per tile of PU_TILE positions, eight rounds of a lane per position (the rows of a round
// are 2 KB in a row): the tiles' sums of `diff`, an exclusive scan over them (cl_scan_u32_u64; modulo 2^32 its low words are the
// running sums), then inside the tile a wave prefix sum per round; the fold adds it to `match`, fills `ref` from the piece that
// pile_ref_place names, and reduces the totals by wave, one 64-bit atomic per wave and total at the wave's end.
// k_pileup_sites<FILL>: the same tiles, a lane per position, ONE body in two instantiations so that the count and the fill cannot
// disagree: FILL = false writes a tile's number of sites, a prefix sum over the tiles places them, FILL = true stores site k of the
// tile (its rank from a ballot) at off[tile] + k: the compaction is stable, sites come out in genome order, and the scratch is 12 bytes
// per 512 positions and not per position.
//
// Bounds by construction, in the terms of es_wave.hpp, and: a table position is formed only from a cursor already checked against
// cur.len (del / match / subst: c < len; anchor: c + L <= len; an insertion run: pile_ins_left's own conditions, 1 <= c <= len forward,
// c < len reversed), only on a reference id < n_pseudo, whose length cl_pileup_create has found equal to the geometry's piece length
// before the first launch; cl_pileup_add takes no arena but that one.  So origin[id] + p < n_pos for every p < len and a + L <= n_pos,
// and diff has n_pos + 1 entries.  The fold and the sites run over x < n_pos alone; pile_ref_place names a piece of the geometry and an
// offset inside it; a site is stored only at off[tile] + k for a flagged position, and the host has checked the total against the
// buffer it made before the fill is launched.  A malformed stream gives its read an error code, the call is CL_E_INVALID — and the
// table keeps what the tuples before it added, so the object is spoiled.
#include "common.hpp"
#include "objects.hpp"
#include "compressor.hpp"
#include "es_wave.hpp"
#include "pileup.hpp"
#include <algorithm>
#include <atomic>

struct cl_pileup {
	cl_ctx* ctx = nullptr; const cl_reads* refs = nullptr;
	std::vector<uint32_t> piece_first, origin; std::vector<uint64_t> seq_base;
	DevBuf<uint64_t> d_seq_base; DevBuf<uint32_t> d_piece_first, d_origin;
	DevBuf<uint32_t> cols, diff; DevBuf<unsigned long long> sums;            // n_pos * PU_COLS; n_pos + 1; PU_SUMS
	PileGeom G{};                                                              // over the device tables
	std::atomic<bool> finished{ false }, spoiled{ false };
};

namespace {
__device__ __forceinline__ unsigned long long pu_wave_sum64(unsigned long long v)
{
#pragma unroll
	for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
	return v;
}

// one read by one wave: the n > 0 stream bytes at s.  Returns the error code (uniform); unplaced = its insertion runs on genome pieces
// that have no position, touched = a tuple of it was met on a genome piece.
__device__ inline uint32_t pu_read(const Arena& R, const PileGeom& G, const uint8_t* __restrict__ s, uint64_t n, uint32_t lane, uint32_t* __restrict__ cols, uint32_t* __restrict__ diff,
                                   uint32_t& unplaced, bool& touched)
{
	uint32_t err = EDE_NONE, lane_err = EDE_NONE;                               // uniform; what a tuple of mine ran into
	const EsStart st = es_start(s, n, lane, R.n);
	unplaced = 0; touched = false;
	if (st.plain) lane_err = es_plain_check(s, n, lane);                       // a plain read lies on no reference
	else if (st.err) err = st.err;
	else
	{
		EsRefs<true> F(R, st);
		bool on = F.cur.id < G.n_pseudo;                                        // the current reference is a genome piece (uniform) ...
		uint64_t origin = on ? G.origin[F.cur.id] : 0;                          // ... that starts here in the table
		bool last_ins = false;                                                  // across windows: the last tuple was an ins
		uint64_t pos = 5;
		while (!err && pos < n)
		{
			const EsWindow W = es_window(s, pos, n, lane);
			if (W.err) { err = W.err; break; }
			const uint32_t b = W.b, t = W.t, v28 = W.v28, adv = es_ref_adv(W); const uint64_t starts = W.starts;
			const uint64_t mI = starts & __ballot(t == T_INS);
			const uint64_t opens = mI & ~((mI << 1) | (last_ins ? 1ull : 0ull));      // ins tuples whose tuple before is no ins
			const uint64_t sw = starts & (W.m5 | __ballot(t == T_MAIN_REF));      // tuples that change the reference
			if (W.is_start && t == T_INS && (b & 0xf) > 3) lane_err = EDE_VALUE;
			uint64_t todo = starts;
			while (todo && !err)
			{	// a stretch of tuples on one reference, then the tuple that ends it
				const EsStretch x = es_stretch(todo, sw);
				const uint64_t seg = x.seg; const uint32_t sl = x.sl;
				if (seg)
				{
					const bool in_seg = (seg >> lane) & 1;
					const uint32_t ad = in_seg ? adv : 0u;                      // (at most 16 multi-byte tuples of 28 bits: the sums fit 32 bits)
					const uint32_t ai = wave_incl_scan(ad);
					const uint32_t atot = __builtin_amdgcn_readfirstlane(__shfl(ai, 63, 64));
					bool no_place = false;
					if (in_seg)
					{
						const uint64_t c = F.cursor + (ai - ad);                // the cursor in front of my tuple
						const uint32_t len = F.cur.len; const bool rev = F.cur.rev;
						if (t == T_DEL || t == T_MATCH || t == T_SUBST)
						{
							if (c >= len) lane_err = EDE_GUARD;
							else if (t == T_SUBST && (b & 0xf) > 2) lane_err = EDE_VALUE;
							else if (on)
							{
								uint32_t ch = t == T_DEL ? (uint32_t)PU_DEL : (uint32_t)PU_MATCH;
								if (t == T_SUBST) ch = PU_SUB + pile_sub_base(ref_base(R, F.cur, c) & 3u, b & 0xf, rev);
								atomicAdd(cols + pile_at(origin, len, rev, c) * PU_COLS + ch, 1u);
							}
						}
						else if (t == T_ANCHOR)
						{
							if (c + v28 > len) lane_err = EDE_GUARD;
							else if (on && v28)
							{
								const uint64_t a = pile_anchor_start(origin, len, rev, c, v28);
								atomicAdd(diff + a, 1u); atomicAdd(diff + a + v28, 0xffffffffu);
							}
						}
						else if (t == T_INS && on && !lane_err && ((opens >> lane) & 1))
						{
							uint64_t p = 0;
							if (pile_ins_left(origin, len, rev, c, p)) atomicAdd(cols + p * PU_COLS + PU_INS, 1u); else no_place = true;
						}
					}
					unplaced += (uint32_t)__popcll(__ballot(no_place));
					if (on) touched = true;
					F.cursor += atot;
				}
				if (sl >= 64) break;
				// the tuple that ends the stretch: an error of a tuple in front of it comes first (the host form meets it first)
				if ((err = es_lane_err(lane < sl ? lane_err : (uint32_t)EDE_NONE))) break;
				if (__shfl(t, sl, 64) == T_MAIN_REF) F.to_main();
				else if ((err = F.to_alt(R, W, sl, lane))) break;
				on = F.cur.id < G.n_pseudo; origin = on ? G.origin[F.cur.id] : 0;      // (F.cur.id < R.n: checked where the id was met)
				todo = es_behind(todo, sl);
			}
			if (err) break;
			last_ins = (mI >> (63u - (uint32_t)__builtin_clzll(starts))) & 1;      // (a window without an error holds a tuple start)
			pos += W.p;
			err = es_lane_err(lane_err);
		}
	}
	if (!err) err = es_lane_err(lane_err);
	return __builtin_amdgcn_readfirstlane(err);
}

// Blocks stride over quads of reads, one wave each.  The first malformed read into *g_err as ~(read << 32 | code) (0: none).
__global__ __launch_bounds__(256) void k_pileup_walk(Arena R, PileGeom G, const uint8_t* __restrict__ es, const uint64_t* __restrict__ es_off, uint32_t n_reads,
                                                     uint32_t* __restrict__ cols, uint32_t* __restrict__ diff, unsigned long long* __restrict__ sums, unsigned long long* __restrict__ g_err)
{
	const uint32_t w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;      // (the wave's number is uniform: said so, the read's offsets are scalar loads)
	for (uint64_t r64 = (uint64_t)blockIdx.x * 4 + w; r64 < n_reads; r64 += (uint64_t)gridDim.x * 4)      // (wave-uniform)
	{
		const uint32_t r = (uint32_t)r64;
		const uint64_t a = es_off[r], e = es_off[r + 1], len = e > a ? e - a : 0;
		uint32_t unplaced = 0; bool touched = false;
		const uint32_t err = len ? pu_read(R, G, es + a, len, lane, cols, diff, unplaced, touched) : (uint32_t)EDE_EMPTY;
		if (lane == 0)
		{
			if (err) atomicMax(g_err, ~(((unsigned long long)r << 32) | err));
			else
			{
				if (unplaced) atomicAdd(sums + PU_S_UNPLACED, (unsigned long long)unplaced);
				if (touched) atomicAdd(sums + PU_S_READS, 1ULL);
			}
		}
	}
}

// tile_sum[tile] = the sum of diff over the tile's positions, modulo 2^32
__global__ __launch_bounds__(256) void k_pileup_tile_sums(const uint32_t* __restrict__ diff, uint64_t n_pos, uint64_t n_tiles, uint32_t* __restrict__ tile_sum)
{
	const uint32_t w = threadIdx.x >> 6, lane = threadIdx.x & 63;
	for (uint64_t tile = (uint64_t)blockIdx.x * 4 + w; tile < n_tiles; tile += (uint64_t)gridDim.x * 4)
	{
		uint32_t v = 0;
#pragma unroll
		for (uint32_t k = 0; k < PU_TILE / 64; ++k) { const uint64_t x = tile * PU_TILE + k * 64 + lane; if (x < n_pos) v += diff[x]; }
		v = wave_sum(v);
		if (lane == 0) tile_sum[tile] = v;
	}
}

// the fold of one tile by one wave: tile_off[tile] = the running sum of diff in front of it (its low 32 bits count)
__global__ __launch_bounds__(256) void k_pileup_fold(Arena R, PileGeom G, uint32_t* __restrict__ cols, const uint32_t* __restrict__ diff, const uint64_t* __restrict__ tile_off, uint64_t n_tiles,
                                                     unsigned long long* __restrict__ sums)
{
	const uint32_t w = threadIdx.x >> 6, lane = threadIdx.x & 63;
	unsigned long long covered = 0, m = 0, sb = 0, dl = 0, in = 0;
	for (uint64_t tile = (uint64_t)blockIdx.x * 4 + w; tile < n_tiles; tile += (uint64_t)gridDim.x * 4)
	{
		uint32_t run = (uint32_t)tile_off[tile];
		for (uint32_t k = 0; k < PU_TILE / 64; ++k)
		{
			const uint64_t x = tile * PU_TILE + k * 64 + lane;
			const bool valid = x < G.n_pos;
			const uint32_t incl = wave_incl_scan(valid ? diff[x] : 0u);
			const uint32_t cov = run + incl;
			run += __shfl(incl, 63, 64);
			if (!valid) continue;
			uint4* row = reinterpret_cast<uint4*>(cols + x * PU_COLS);
			uint4 a = row[0], b = row[1];
			a.x += cov;
			uint32_t id, off; pile_ref_place(G, x, id, off);                    // (a piece of the geometry, an offset inside it)
			RefCursor c; c.id = id; c.len = R.lens[id]; c.wo = R.word_off[id]; c.rev = false;
			b.w = ref_base(R, c, off) & 3u;
			row[0] = a; row[1] = b;
			const unsigned long long sub = (unsigned long long)a.y + a.z + a.w + b.x;
			covered += (a.x || sub || b.y) ? 1u : 0u; m += a.x; sb += sub; dl += b.y; in += b.z;
		}
	}
	covered = pu_wave_sum64(covered); m = pu_wave_sum64(m); sb = pu_wave_sum64(sb); dl = pu_wave_sum64(dl); in = pu_wave_sum64(in);
	if (lane == 0)
	{
		if (covered) atomicAdd(sums + PU_S_COVERED, covered);
		if (m) atomicAdd(sums + PU_S_MATCH, m);
		if (sb) atomicAdd(sums + PU_S_SUB, sb);
		if (dl) atomicAdd(sums + PU_S_DEL, dl);
		if (in) atomicAdd(sums + PU_S_INS, in);
	}
}

// FILL = false: tile_cnt[tile] = its sites.  FILL = true: site k of the tile at out + off[tile] + k, three 16-byte stores.
template<bool FILL> __global__ __launch_bounds__(256) void k_pileup_sites(PileGeom G, const uint32_t* __restrict__ cols, PileThresholds T, uint64_t n_tiles, uint32_t* __restrict__ tile_cnt,
                                                                          const uint64_t* __restrict__ off, cl_pileup_site* __restrict__ out)
{
	const uint32_t w = threadIdx.x >> 6, lane = threadIdx.x & 63;
	for (uint64_t tile = (uint64_t)blockIdx.x * 4 + w; tile < n_tiles; tile += (uint64_t)gridDim.x * 4)
	{
		uint32_t cnt = 0;
		const uint64_t o0 = FILL ? off[tile] : 0;
		for (uint32_t k = 0; k < PU_TILE / 64; ++k)
		{
			const uint64_t x = tile * PU_TILE + k * 64 + lane;
			cl_pileup_site o; bool is = false;
			if (x < G.n_pos)
			{
				const uint4* row = reinterpret_cast<const uint4*>(cols + x * PU_COLS);
				const uint4 a = row[0], b = row[1];
				const uint32_t col[PU_COLS] = { a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w };
				is = pile_site(G, x, col, T, o);
			}
			const uint64_t mask = __ballot(is);
			if (FILL && is)
			{
				uint4* dst = reinterpret_cast<uint4*>(out + o0 + cnt + (uint32_t)__popcll(mask & ((1ull << lane) - 1)));
				dst[0] = make_uint4(o.seq, o.pos, o.ref, o.kind); dst[1] = make_uint4(o.match, o.sub[0], o.sub[1], o.sub[2]); dst[2] = make_uint4(o.sub[3], o.del, o.ins, o.depth);
			}
			cnt += (uint32_t)__popcll(mask);
		}
		if (!FILL && lane == 0) tile_cnt[tile] = cnt;
	}
}

inline uint32_t tile_grid(const cl_ctx* ctx, uint64_t n_tiles) { return (uint32_t)std::min<uint64_t>((n_tiles + 3) / 4, 8ull * (uint64_t)std::max(1, ctx->n_cu)); }
inline Arena arena_of(const cl_reads* refs) { return Arena{ refs->packed.p, nullptr, refs->word_off.p, refs->lens.p, refs->n_reads }; }
} // namespace

extern "C" cl_status cl_pileup_create(cl_ctx* ctx, const cl_reads* refs, const uint64_t* h_seq_len, uint32_t n_seqs, uint32_t read_len, uint32_t overlap, cl_pileup** out)
{
	if (out) *out = nullptr;
	if (!ctx || !refs || !out) return cl_fail(ctx, CL_E_INVALID, "cl_pileup_create: null argument");
	std::unique_ptr<cl_pileup> p(new cl_pileup);
	p->ctx = ctx; p->refs = refs;
	const cl_status s = pile_geometry(h_seq_len, n_seqs, read_len, overlap, p->piece_first, p->seq_base, p->origin);
	if (s == CL_E_UNSUPPORTED) return cl_fail(ctx, s, "cl_pileup_create: a sequence of 2^32 bases or more, 2^32 pieces or more, or a table of 2^32 positions or more");
	if (s != CL_OK) return cl_fail(ctx, s, "cl_pileup_create: the piece length must exceed the overlap, and sequences need their lengths");
	const uint32_t n_pseudo = p->piece_first[n_seqs]; const uint64_t n_pos = p->seq_base[n_seqs];
	if (n_pseudo > refs->n_reads) return cl_fail(ctx, CL_E_INVALID, "cl_pileup_create: the geometry gives " + std::to_string(n_pseudo) + " pieces, the arena has " + std::to_string(refs->n_reads) + " reads");
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	if (n_pseudo)
	{	// cur.len of a piece in the walk IS the geometry's piece length: every table position it forms lies inside the table
		std::vector<uint32_t> lens(n_pseudo);
		HIP_TRY(ctx, hipMemcpyAsync(lens.data(), refs->lens.p, (uint64_t)n_pseudo * 4, hipMemcpyDeviceToHost, cl_launch_stream(ctx)));
		HIP_TRY(ctx, hipStreamSynchronize(cl_launch_stream(ctx)));
		for (uint32_t q = 0; q < n_seqs; ++q)
			for (uint32_t i = p->piece_first[q]; i < p->piece_first[q + 1]; ++i)
			{
				const uint64_t want = pile_piece_len(h_seq_len, p->piece_first, q, i, read_len, overlap);
				if (lens[i] != want) return cl_fail(ctx, CL_E_INVALID, "cl_pileup_create: pseudo read " + std::to_string(i) + " has " + std::to_string(lens[i]) + " bases, the geometry gives " + std::to_string(want));
			}
	}
	const uint64_t bytes = n_pos * PU_COLS * 4 + (n_pos + 1) * 4;
	if (p->cols.alloc(ctx, n_pos * PU_COLS) != hipSuccess || p->diff.alloc(ctx, n_pos + 1) != hipSuccess)
	{
		(void)hipGetLastError();
		return cl_fail(ctx, CL_E_NOMEM, "cl_pileup_create: the table of " + std::to_string(n_pos) + " positions needs " + std::to_string(bytes) + " bytes of device memory");
	}
	DEV_ALLOC(ctx, p->sums, PU_SUMS); DEV_ALLOC(ctx, p->d_seq_base, (uint64_t)n_seqs + 1); DEV_ALLOC(ctx, p->d_piece_first, (uint64_t)n_seqs + 1); DEV_ALLOC(ctx, p->d_origin, n_pseudo);
	hipStream_t st = cl_launch_stream(ctx);
	if (n_pos) HIP_TRY(ctx, hipMemsetAsync(p->cols.p, 0, n_pos * PU_COLS * 4, st));
	HIP_TRY(ctx, hipMemsetAsync(p->diff.p, 0, (n_pos + 1) * 4, st));
	HIP_TRY(ctx, hipMemsetAsync(p->sums.p, 0, PU_SUMS * 8, st));
	HIP_TRY(ctx, hipMemcpyAsync(p->d_seq_base.p, p->seq_base.data(), ((uint64_t)n_seqs + 1) * 8, hipMemcpyHostToDevice, st));
	HIP_TRY(ctx, hipMemcpyAsync(p->d_piece_first.p, p->piece_first.data(), ((uint64_t)n_seqs + 1) * 4, hipMemcpyHostToDevice, st));
	if (n_pseudo) HIP_TRY(ctx, hipMemcpyAsync(p->d_origin.p, p->origin.data(), (uint64_t)n_pseudo * 4, hipMemcpyHostToDevice, st));
	HIP_TRY(ctx, hipStreamSynchronize(st));
	p->G = PileGeom{ p->d_seq_base.p, p->d_piece_first.p, p->d_origin.p, n_pos, n_seqs, n_pseudo, read_len, read_len - overlap };
	*out = p.release();
	return CL_OK;
}
extern "C" void cl_pileup_free(cl_pileup* p) { delete p; }
extern "C" uint64_t cl_pileup_positions(const cl_pileup* p) { return p ? p->G.n_pos : 0; }

// the streams of a batch added by a launch on `ctx`: the object's own context, or that of the encode lane which made the streams
static cl_status pile_add_on(cl_ctx* ctx, cl_pileup* p, const cl_reads* refs, const uint8_t* d_es, const uint64_t* d_es_off, uint32_t n_reads, uint32_t max_blocks)
{
	if (!p || !refs || (n_reads && (!d_es || !d_es_off))) return cl_fail(ctx, CL_E_INVALID, "cl_pileup_add: null argument");
	if (p->spoiled) return cl_fail(ctx, CL_E_INVALID, "cl_pileup_add: the table is spoiled by a malformed stream of an earlier call");
	if (p->finished) return cl_fail(ctx, CL_E_INVALID, "cl_pileup_add: called after cl_pileup_finish");
	if (refs != p->refs) return cl_fail(ctx, CL_E_INVALID, "cl_pileup_add: not the arena the table was created for");
	if (!n_reads) return CL_OK;
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	if (!max_blocks) max_blocks = 4 * (uint32_t)std::max(1, ctx->n_cu);
	const uint32_t grid = std::min(grid_for(n_reads, 4), max_blocks);
	DevBuf<unsigned long long> g; DEV_ALLOC(ctx, g, 1);
	HIP_TRY(ctx, hipMemsetAsync(g.p, 0, 8, cl_launch_stream(ctx)));
	LAUNCH(ctx, k_pileup_walk, grid, 256, arena_of(refs), p->G, d_es, d_es_off, n_reads, p->cols.p, p->diff.p, p->sums.p, g.p);
	HIP_TRY(ctx, hipGetLastError());
	unsigned long long h_err = 0;
	HIP_TRY(ctx, hipMemcpyAsync(&h_err, g.p, 8, hipMemcpyDeviceToHost, cl_launch_stream(ctx)));
	HIP_TRY(ctx, hipStreamSynchronize(cl_launch_stream(ctx)));
	cl_timing_collect(ctx);
	if (h_err)
	{
		p->spoiled = true;
		const uint64_t key = ~(uint64_t)h_err;
		return cl_fail(ctx, CL_E_INVALID, "cl_pileup_add: malformed tuple stream, first: read " + std::to_string(key >> 32) + ": " + ed_error_text((uint32_t)key) + " (the table is spoiled)");
	}
	return CL_OK;
}
extern "C" cl_status cl_pileup_add(cl_pileup* p, const cl_reads* refs, const uint8_t* d_es, const uint64_t* d_es_off, uint32_t n_reads, uint32_t max_blocks)
{
	return p ? pile_add_on(p->ctx, p, refs, d_es, d_es_off, n_reads, max_blocks) : CL_E_INVALID;
}

extern "C" cl_status cl_pileup_finish(cl_pileup* p)
{
	if (!p) return CL_E_INVALID;
	cl_ctx* ctx = p->ctx;
	if (p->spoiled) return cl_fail(ctx, CL_E_INVALID, "cl_pileup_finish: the table is spoiled by a malformed stream of an earlier call");
	if (p->finished) return cl_fail(ctx, CL_E_INVALID, "cl_pileup_finish: called twice");
	p->finished = true;                                                         // (adds are refused from here on, whatever happens below)
	const uint64_t n_pos = p->G.n_pos, n_tiles = (n_pos + PU_TILE - 1) / PU_TILE;
	if (!n_tiles) return CL_OK;
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	DevBuf<uint32_t> tile_sum; DevBuf<uint64_t> tile_off;
	DEV_ALLOC(ctx, tile_sum, n_tiles); DEV_ALLOC(ctx, tile_off, n_tiles + 1);
	const uint32_t grid = tile_grid(ctx, n_tiles);
	LAUNCH(ctx, k_pileup_tile_sums, grid, 256, (const uint32_t*)p->diff.p, n_pos, n_tiles, tile_sum.p);
	HIP_TRY(ctx, hipGetLastError());
	CL_TRY(cl_scan_u32_u64(ctx, tile_sum.p, tile_off.p, n_tiles, nullptr));      // (no total asked for: the sums count modulo 2^32 only)
	LAUNCH(ctx, k_pileup_fold, grid, 256, arena_of(p->refs), p->G, p->cols.p, (const uint32_t*)p->diff.p, (const uint64_t*)tile_off.p, n_tiles, p->sums.p);
	HIP_TRY(ctx, hipGetLastError());
	HIP_TRY(ctx, hipStreamSynchronize(cl_launch_stream(ctx)));
	cl_timing_collect(ctx);
	p->refs = nullptr;                                                          // (the arena is not needed any more)
	return CL_OK;
}

static cl_status pile_ready(const cl_pileup* p, const char* who)
{
	if (p->spoiled) return cl_fail(p->ctx, CL_E_INVALID, std::string(who) + ": the table is spoiled by a malformed stream of an earlier call");
	if (!p->finished) return cl_fail(p->ctx, CL_E_INVALID, std::string(who) + ": call after cl_pileup_finish");
	return CL_OK;
}
extern "C" cl_status cl_pileup_columns(const cl_pileup* p, uint64_t first, uint64_t n, uint32_t* h_out)
{
	if (!p) return CL_E_INVALID;
	cl_ctx* ctx = p->ctx;
	CL_TRY(pile_ready(p, "cl_pileup_columns"));
	if (first > p->G.n_pos || n > p->G.n_pos - first || (n && !h_out)) return cl_fail(ctx, CL_E_INVALID, "cl_pileup_columns: positions outside the table, or no room for them");
	if (!n) return CL_OK;
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	HIP_TRY(ctx, hipMemcpyAsync(h_out, p->cols.p + first * PU_COLS, n * PU_COLS * 4, hipMemcpyDeviceToHost, cl_launch_stream(ctx)));
	HIP_TRY(ctx, hipStreamSynchronize(cl_launch_stream(ctx)));
	return CL_OK;
}
extern "C" cl_status cl_pileup_totals(const cl_pileup* p, cl_pileup_sums* out)
{
	if (!p || !out) return CL_E_INVALID;
	cl_ctx* ctx = p->ctx;
	CL_TRY(pile_ready(p, "cl_pileup_totals"));
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	HIP_TRY(ctx, hipMemcpyAsync(out, p->sums.p, sizeof(*out), hipMemcpyDeviceToHost, cl_launch_stream(ctx)));
	HIP_TRY(ctx, hipStreamSynchronize(cl_launch_stream(ctx)));
	return CL_OK;
}
extern "C" cl_status cl_pileup_sites(const cl_pileup* p, uint32_t min_depth, uint32_t min_alt, uint32_t min_permille, cl_pileup_site* h_out, uint64_t cap, uint64_t* n_out)
{
	if (n_out) *n_out = 0;
	if (!p || !n_out) return CL_E_INVALID;
	cl_ctx* ctx = p->ctx;
	CL_TRY(pile_ready(p, "cl_pileup_sites"));
	const uint64_t n_tiles = (p->G.n_pos + PU_TILE - 1) / PU_TILE;
	if (!n_tiles) return CL_OK;
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	const PileThresholds T{ min_depth, min_alt, min_permille };
	DevBuf<uint32_t> tile_cnt; DevBuf<uint64_t> off; DevBuf<cl_pileup_site> out;
	DEV_ALLOC(ctx, tile_cnt, n_tiles); DEV_ALLOC(ctx, off, n_tiles + 1);
	const uint32_t grid = tile_grid(ctx, n_tiles);
	LAUNCH(ctx, k_pileup_sites<false>, grid, 256, p->G, (const uint32_t*)p->cols.p, T, n_tiles, tile_cnt.p, (const uint64_t*)nullptr, (cl_pileup_site*)nullptr);
	HIP_TRY(ctx, hipGetLastError());
	uint64_t total = 0;
	CL_TRY(cl_scan_u32_u64(ctx, tile_cnt.p, off.p, n_tiles, &total));
	*n_out = total;
	if (total > cap || (total && !h_out)) { cl_timing_collect(ctx); return cl_fail(ctx, CL_E_CAPACITY, "cl_pileup_sites: need " + std::to_string(total) + " records"); }
	if (total)
	{	// (off[n_tiles] = total = the records of `out`: no site of the fill lies outside it)
		DEV_ALLOC(ctx, out, total);
		LAUNCH(ctx, k_pileup_sites<true>, grid, 256, p->G, (const uint32_t*)p->cols.p, T, n_tiles, (uint32_t*)nullptr, (const uint64_t*)off.p, out.p);
		HIP_TRY(ctx, hipGetLastError());
		HIP_TRY(ctx, hipMemcpyAsync(h_out, out.p, total * sizeof(cl_pileup_site), hipMemcpyDeviceToHost, cl_launch_stream(ctx)));
		HIP_TRY(ctx, hipStreamSynchronize(cl_launch_stream(ctx)));
	}
	cl_timing_collect(ctx);
	return CL_OK;
}

extern "C" cl_status cl_pileup_host(const uint8_t* h_ref_codes, const uint64_t* h_ref_off, uint32_t n_refs, const uint64_t* h_seq_len, uint32_t n_seqs, uint32_t read_len, uint32_t overlap,
                                    const uint8_t* h_es, const uint64_t* h_es_off, uint64_t n_reads, uint32_t min_depth, uint32_t min_alt, uint32_t min_permille,
                                    uint32_t* h_cols, cl_pileup_site* h_sites, uint64_t cap, uint64_t* n_sites, cl_pileup_sums* sums, uint64_t* bad_read, uint32_t* bad_code)
{
	if (n_sites) *n_sites = 0;
	if (bad_read) *bad_read = 0;
	if (bad_code) *bad_code = 0;
	if (!n_sites || !sums || (n_refs && (!h_ref_off || !h_ref_codes))) return CL_E_INVALID;
	PileHost H;
	CL_TRY(H.init(h_seq_len, n_seqs, read_len, overlap));
	if (H.G.n_pseudo > n_refs) return CL_E_INVALID;
	for (uint32_t s = 0; s < n_seqs; ++s)
		for (uint32_t i = H.piece_first[s]; i < H.piece_first[s + 1]; ++i)
			if (h_ref_off[i + 1] - h_ref_off[i] != pile_piece_len(h_seq_len, H.piece_first, s, i, read_len, overlap)) return CL_E_INVALID;
	if (!pile_add_host(H, h_ref_codes, h_ref_off, n_refs, h_es, h_es_off, n_reads, bad_read, bad_code)) return CL_E_INVALID;
	pile_fold_host(H, h_ref_codes, h_ref_off);
	std::vector<cl_pileup_site> S;
	pile_sites_host(H, PileThresholds{ min_depth, min_alt, min_permille }, S);
	*n_sites = S.size(); *sums = H.sums;
	if (h_cols && !H.cols.empty()) memcpy(h_cols, H.cols.data(), H.cols.size() * 4);
	if (S.size() > cap || (!S.empty() && !h_sites)) return CL_E_CAPACITY;
	if (!S.empty()) memcpy(h_sites, S.data(), S.size() * sizeof(cl_pileup_site));
	return CL_OK;
}

extern "C" void cl_ctx_set_pileup(cl_ctx* c, int on) { if (c) c->pileup = on != 0; }

// Internal (pass_steps.hpp: tuple_streams): one batch of tuple streams added to the compressor's table, by a launch on the context that made them
cl_status pileup_chunk(cl_ctx* ctx, cl_pileup* p, const cl_reads* refs, const uint8_t* d_es, const uint64_t* d_es_off, uint32_t n_reads)
{
	if (!p) return cl_fail(ctx, CL_E_INVALID, "cl_ctx_set_pileup: no table (the flag was off when cl_compressor_refs_finish ran, or cl_compress_shard)");
	return pile_add_on(ctx, p, refs, d_es, d_es_off, n_reads, 0);
}
// Internal (stream.hip: cl_compressor_refs_finish): the compressor's table, from the geometry kept for the mappings, over its reference arena
cl_status pileup_for_compressor(cl_compressor* c)
{
	return cl_pileup_create(c->ctx, c->refs, c->map_seq_len_h.data(), (uint32_t)c->map_seq_len_h.size(), c->map_geom.read_len, c->map_geom.read_len - c->map_geom.step, &c->pileup);
}
extern "C" cl_status cl_compressor_pileup(cl_compressor* c, cl_pileup** out)
{
	if (out) *out = nullptr;
	if (!c || !out) return CL_E_INVALID;
	cl_ctx* ctx = c->ctx;
	if (!c->pileup) return cl_fail(ctx, CL_E_INVALID, "cl_compressor_pileup: no table (cl_ctx_set_pileup was off when cl_compressor_refs_finish ran)");
	if (c->phase != 2 || c->enc_chunk != c->chunk_reads.size()) return cl_fail(ctx, CL_E_INVALID, "cl_compressor_pileup: call after the last cl_compressor_encode");
	if (!c->pileup->finished && !c->pileup->spoiled) CL_TRY(cl_pileup_finish(c->pileup));
	CL_TRY(pile_ready(c->pileup, "cl_compressor_pileup"));
	*out = c->pileup;
	return CL_OK;
}
