// cigars.hip — the base-level CIGAR of every overlap record on the device (cigars.hpp): cl_cigars_of over the tuple streams
// that cl_encode_reads wrote; the host twin's C entry; the pipeline's hook (cigars_chunk, called by mappings_chunk) and what a context keeps.
//
// k_cigar_walk<FILL> walks the streams as k_overlap_walk does (es_wave.hpp): ONE WAVE PER READ, the stream 64 bytes per window, the window
// cut into stretches on one reference, persistent blocks of four waves over the reads; no LDS, no barrier.  Inside a stretch every
// tuple-start lane knows its operation and length (cg_tuple).  A lane is a RUN HEAD when its operation differs from that of the nearest
// operation-bearing lane below it — the open run's, carried in, for the lowest —: one ballot.  A run's length is a segmented wave sum, the
// difference of an inclusive scan of the lengths at two heads; its index in the record a prefix count of the heads.  Every head closes the
// run in front of it and stores that run's word, a lane per run, neighbouring lanes to neighbouring words; the last run of a stretch stays
// open.  Carried uniformly across stretches and windows: the open run (operation, length, its index = the runs closed so far) and `count`,
// the runs up to and including the one that holds the visit's LAST ALIGNED COLUMN so far.  Runs at or past `count` are the insertions and
// deletions behind that column: they become part of the record only when another aligned column of the visit follows, which moves `count`
// past them — in this window or in any later one.  The count pass (FILL = false) writes `count` of the k-th visit of read r at
// rec_off[r] + k; a prefix sum over the records gives op_off; the fill (FILL = true, ONE body, so that the two cannot disagree) loads the
// record's count when the visit meets its first aligned column and stores run j at op_off[rec] + j only while j is below that count — a run
// at or past it is by construction a trimmed one.  So a run is stored at most once, by the lane that closes it, no store depends on another
// and the kernel loads nothing that it stored.  What lies in front of a visit's first aligned column is masked off where that column is met.
// A visit on a reference id at or past id_limit gets the count 0, and with it no store.
//
// Bounds by construction, in the terms of es_wave.hpp: every loop bound is known before the loop (a window is the min(64, bytes left) bytes
// in front of es_off[r + 1]; the tuple-start loop and the stretch loop run over at most 64 bits of a mask; the read loop over n_reads);
// a window never holds a byte at or past es_off[r + 1] and a tuple that would cross it is an error; every reference id is checked against
// the arena's read count before lens[] is indexed with it; no reference base is loaded.  Stores: a count only at rec_off[r] + k while that
// is below rec_off[r + 1], and rec_off[n_reads] records were allocated; an operation only at op_off[rec] + j with j < rec_ops[rec], which
// lies below op_off[rec + 1] <= op_off[n_rec], the total that the host has checked against the capacity before the fill is launched.
// A malformed stream gives its read an error code; the call is CL_E_INVALID and hands nothing out.
#include "common.hpp"
#include "objects.hpp"
#include "es_wave.hpp"
#include "cigars.hpp"
#include "cigar_coder.hpp"
#include "compressor.hpp"
#include <algorithm>
#include <mutex>

namespace {
constexpr uint32_t CG_NONE = 0xffffffffu;
// the open visit (uniform).  has: it has met an aligned column, and from there on a run is open: open_op / open_len, its index = closed.
struct CgVisit { bool has = false; uint32_t open_op = 0, closed = 0, count = 0, viol = CG_NONE, cnt = 0; uint64_t open_len = 0, base = 0; };
struct CgOut { const uint64_t* rec_off; uint32_t* rec_ops_out; const uint32_t* rec_ops; const uint64_t* op_off; uint32_t* ops; };

// the open visit closed: a record if it holds an aligned column.  Uniform; lane 0 stores the count (count pass) or the open run (fill).
template<bool FILL> __device__ inline void cg_close(CgVisit& V, uint32_t& n_rec, bool& too_long, uint32_t ref_id, uint32_t id_limit, uint32_t lane, const CgOut& O, uint64_t r0, uint64_t r1)
{
	if (V.has)
	{
		uint32_t w = 0;
		const bool kept = V.closed < V.count;                                  // the open run holds the last aligned column, or lies behind it
		if (kept && !cg_word(V.open_op, V.open_len, w)) V.viol = V.viol < V.closed ? V.viol : V.closed;
		if (V.viol < V.count) too_long = true;
		if (lane == 0 && r0 + n_rec < r1)
		{
			if (!FILL) O.rec_ops_out[r0 + n_rec] = ref_id < id_limit ? V.count : 0u;
			else if (V.closed < V.cnt) O.ops[V.base + V.closed] = w;              // (cnt <= count: the run is a kept one)
		}
		++n_rec;
	}
	V = CgVisit();
}

// one read by one wave: the n > 0 stream bytes at s.  Returns the error code (uniform); n_rec = its records.
template<bool FILL> __device__ inline uint32_t cg_read(const Arena& A, const uint8_t* __restrict__ s, uint64_t n, uint32_t lane, uint32_t id_limit, const CgOut& O, uint64_t r0, uint64_t r1, uint32_t& n_rec)
{
	uint32_t err = EDE_NONE, lane_err = EDE_NONE;                               // uniform; what a tuple of mine ran into
	const EsStart st = es_start(s, n, lane, A.n);
	uint64_t qpos = 0;
	bool too_long = false;
	n_rec = 0;
	if (st.plain)
	{	// the rest of the stream is `plain` tuples, a lane per base: no record, the same checks as the overlaps'
		lane_err = es_plain_check(s, n, lane);
		qpos = n - 1;
	}
	else if (st.err) err = st.err;
	else
	{
		EsRefs<false> F(A, st);
		CgVisit V;
		uint64_t pos = 5;
		while (!err && pos < n)
		{
			const EsWindow W = es_window(s, pos, n, lane);
			if (W.err) { err = W.err; break; }
			const uint32_t b = W.b, t = W.t, v28 = W.v28; const uint64_t starts = W.starts; const bool is_start = W.is_start;
			const uint32_t adv = es_ref_adv(W), qadv = es_read_adv(W);
			const uint64_t anch = starts & __ballot(t == T_ANCHOR);
			const uint64_t aligned = starts & __ballot(t == T_MATCH || t == T_SUBST || (t == T_ANCHOR && v28 > 0));
			const uint64_t sw = starts & (W.m5 | __ballot(t == T_MAIN_REF));      // tuples that change the reference
			uint32_t my_len = 0;                                                   // what my tuple contributes
			const uint32_t my_op = is_start ? cg_tuple(t, v28, my_len) : 0u;
			const uint64_t bearing = __ballot(my_len > 0);
			if (is_start)
			{
				if (t == T_INS && (b & 0xf) > 3) lane_err = EDE_VALUE;
				if (t == T_SUBST && (b & 0xf) > 2) lane_err = EDE_VALUE;
			}
			uint64_t todo = starts;
			while (todo && !err)
			{	// a stretch of tuples on one reference, then the tuple that ends it
				const EsStretch x = es_stretch(todo, sw);
				const uint64_t seg = x.seg; const uint32_t sl = x.sl;
				if (seg)
				{
					const bool in_seg = (seg >> lane) & 1;
					const uint32_t ad = in_seg ? adv : 0u, qd = in_seg ? qadv : 0u;    // (at most 16 multi-byte tuples of 28 bits: the sums fit 32 bits)
					const uint32_t ai = wave_incl_scan(ad);
					const uint32_t atot = __builtin_amdgcn_readfirstlane(__shfl(ai, 63, 64)), qtot = __builtin_amdgcn_readfirstlane(__shfl(wave_incl_scan(qd), 63, 64));
					if (in_seg && (t == T_DEL || t == T_MATCH || t == T_SUBST) && F.cursor + (ai - ad) >= F.cur.len) lane_err = lane_err ? lane_err : (uint32_t)EDE_GUARD;
					for (uint64_t am = seg & anch; am; am &= am - 1)
					{	// an anchor: that it lies on its reference
						const uint32_t l = (uint32_t)__builtin_ctzll(am);
						const uint32_t alen = __builtin_amdgcn_readfirstlane(__shfl(v28, l, 64));
						const uint64_t a_c = F.cursor + (__builtin_amdgcn_readfirstlane(__shfl(ai, l, 64)) - alen);
						if (a_c + alen > F.cur.len) { err = EDE_GUARD; break; }
					}
					if (err) break;
					// the operations of the stretch that count: from the visit's first aligned column on
					const uint64_t al = seg & aligned;
					uint64_t ob = seg & bearing;
					if (!V.has) ob = al ? ob & ~((1ull << (uint32_t)__builtin_ctzll(al)) - 1) : 0;
					if (ob)
					{
						if (FILL && !V.has && r0 + n_rec < r1)
						{	// the record this visit is: its count and where its operations go (written by the count pass and the scan, not by this launch)
							V.cnt = O.rec_ops[r0 + n_rec]; V.base = O.op_off[r0 + n_rec];
						}
						const bool mine = (ob >> lane) & 1;
						const uint32_t l32 = mine ? my_len : 0u;
						const uint32_t li = wave_incl_scan(l32), ex = li - l32;
						const uint32_t tot = __builtin_amdgcn_readfirstlane(__shfl(li, 63, 64));
						// run heads: my operation differs from that of the nearest operation-bearing lane below me, the open run's for the lowest
						const uint64_t below = ob & ((1ull << lane) - 1);
						const uint32_t below_op = __shfl(my_op, below ? 63u - (uint32_t)__builtin_clzll(below) : 0u, 64);
						const uint32_t prev_op = below ? below_op : V.has ? V.open_op : 0u;
						const bool is_head = mine && my_op != prev_op;
						const uint64_t heads = __ballot(is_head);
						// a head closes the run in front of it: the one of the head below it, or the open run carried in
						const uint64_t hb = heads & ((1ull << lane) - 1);
						const uint32_t ph = hb ? 63u - (uint32_t)__builtin_clzll(hb) : 0u;
						const uint32_t ex_ph = __shfl(ex, ph, 64), op_ph = __shfl(my_op, ph, 64);
						const bool closes = is_head && (hb || V.has);
						const uint64_t run_len = hb ? (uint64_t)(ex - ex_ph) : V.open_len + ex;
						const uint32_t run_op = hb ? op_ph : V.open_op;
						const uint32_t run_idx = V.closed + (uint32_t)__popcll(hb) - (V.has ? 0u : 1u);      // (for a lane that closes)
						uint32_t w = 0;
						const bool fits = !closes || cg_word(run_op, run_len, w);
						if (FILL && closes && run_idx < V.cnt) O.ops[V.base + run_idx] = w;
						if (const uint64_t badm = __ballot(!fits))
						{	// the lowest run that does not fit: an error only if the record keeps it
							const uint32_t vi = __builtin_amdgcn_readfirstlane(__shfl(run_idx, (uint32_t)__builtin_ctzll(badm), 64));
							V.viol = V.viol < vi ? V.viol : vi;
						}
						// the runs up to the one that holds the last aligned column so far
						if (al) V.count = V.closed + (V.has ? 1u : 0u) + (uint32_t)__popcll(heads & ((2ull << (63u - (uint32_t)__builtin_clzll(al))) - 1));
						if (heads)
						{	// the run of the highest head stays open
							const uint32_t lh = 63u - (uint32_t)__builtin_clzll(heads);
							V.closed += (uint32_t)__popcll(heads) - (V.has ? 0u : 1u);
							V.open_len = tot - __builtin_amdgcn_readfirstlane(__shfl(ex, lh, 64));
							V.open_op = __builtin_amdgcn_readfirstlane(__shfl(my_op, lh, 64));
						}
						else V.open_len += tot;
						V.has = true;
					}
					F.cursor += atot; qpos += qtot;
				}
				if (sl >= 64) break;
				// the tuple that ends the stretch: a position error inside the visit comes first (the host form meets it first)
				if ((err = es_lane_err(lane < sl ? lane_err : (uint32_t)EDE_NONE))) break;
				const bool to_main = __shfl(t, sl, 64) == T_MAIN_REF;
				cg_close<FILL>(V, n_rec, too_long, F.cur.id, id_limit, lane, O, r0, r1);
				if (to_main) F.to_main();
				else if ((err = F.to_alt(A, W, sl, lane))) break;
				todo = es_behind(todo, sl);
			}
			if (err) break;
			pos += W.p;
			err = es_lane_err(lane_err);
		}
		if (!err) cg_close<FILL>(V, n_rec, too_long, F.cur.id, id_limit, lane, O, r0, r1);      // the stream's end closes the last visit
	}
	if (!err) err = es_lane_err(lane_err);
	err = __builtin_amdgcn_readfirstlane(err);
	if (!err && (qpos > OV_POS_MAX || n > OV_POS_MAX)) err = EDE_GUARD;          // as the overlaps; and a record's count is 32 bits (a tuple has a byte at the least)
	if (!err && too_long) err = CGE_RUN;
	return err;
}

// Blocks stride over quads of reads, one wave each.  FILL = false: the counts of read r's records at rec_off[r] .. and the first refused read
// into *g_err as ~(read << 32 | code) (0: none).  FILL = true (after a count without an error): the operations of its records.
template<bool FILL> __global__ __launch_bounds__(256) void k_cigar_walk(Arena A, const uint8_t* __restrict__ es, const uint64_t* __restrict__ es_off, uint32_t n_reads, uint32_t id_limit, CgOut O,
                                                                        unsigned long long* __restrict__ g_err)
{
	const uint32_t w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;      // (the wave's number is uniform: the read's offsets are scalar loads)
	for (uint64_t r64 = (uint64_t)blockIdx.x * 4 + w; r64 < n_reads; r64 += (uint64_t)gridDim.x * 4)      // (wave-uniform)
	{
		const uint32_t r = (uint32_t)r64;
		const uint64_t a = es_off[r], e = es_off[r + 1], len = e > a ? e - a : 0;
		uint32_t nr = 0;
		const uint32_t err = len ? cg_read<FILL>(A, es + a, len, lane, id_limit, O, O.rec_off[r], O.rec_off[r + 1], nr) : (uint32_t)EDE_EMPTY;
		if (!FILL && lane == 0 && err) atomicMax(g_err, ~(((unsigned long long)r << 32) | err));
	}
}

// count, place, fill over the n_reads > 0 streams, with the record offsets of the overlaps' walk over them (d_rec_off, n_rec = their total).
// limit: ids at or past it count nothing.  The counts come in a buffer made here; the operations go to d_ops (cap words), or — with `own` —
// to a buffer made here once the total is known.  CL_E_CAPACITY is the caller's to give: *n_ops = the need, and nothing is filled past cap.
cl_status cg_run(cl_ctx* ctx, const cl_reads* refs, const uint8_t* d_es, const uint64_t* d_es_off, uint32_t n_reads, uint32_t limit, uint32_t max_blocks, const uint64_t* d_rec_off, uint64_t n_rec,
                 DevBuf<uint32_t>& rec_ops, uint32_t* d_ops, uint64_t cap, DevBuf<uint32_t>* own, uint64_t* n_ops, bool* filled)
{
	*n_ops = 0; *filled = false;
	if (n_rec > OV_POS_MAX) return cl_fail(ctx, CL_E_UNSUPPORTED, "cl_cigars_of: 2^32 records or more in one call");
	if (!n_rec) { *filled = true; return CL_OK; }
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	if (!max_blocks) max_blocks = 4 * (uint32_t)std::max(1, ctx->n_cu);
	const uint32_t grid = std::min(grid_for(n_reads, 4), max_blocks);
	DevBuf<uint64_t> op_off; DevBuf<unsigned long long> g;
	DEV_ALLOC(ctx, rec_ops, n_rec); DEV_ALLOC(ctx, op_off, n_rec + 1); DEV_ALLOC(ctx, g, 1);
	HIP_TRY(ctx, hipMemsetAsync(g.p, 0, 8, cl_launch_stream(ctx)));
	const Arena A{ nullptr, nullptr, nullptr, refs->lens.p, refs->n_reads };
	LAUNCH(ctx, k_cigar_walk<false>, grid, 256, A, d_es, d_es_off, n_reads, limit, CgOut{ d_rec_off, rec_ops.p, nullptr, nullptr, nullptr }, g.p);
	HIP_TRY(ctx, hipGetLastError());
	unsigned long long h_err = 0;
	HIP_TRY(ctx, hipMemcpyAsync(&h_err, g.p, 8, hipMemcpyDeviceToHost, cl_launch_stream(ctx)));
	HIP_TRY(ctx, hipStreamSynchronize(cl_launch_stream(ctx)));
	if (h_err)
	{
		cl_timing_collect(ctx);
		const uint64_t key = ~(uint64_t)h_err; const uint32_t code = (uint32_t)key;
		return cl_fail(ctx, code == CGE_RUN ? CL_E_UNSUPPORTED : CL_E_INVALID, std::string("cl_cigars_of: ") + (code == CGE_RUN ? "read " : "malformed tuple stream, first: read ") + std::to_string(key >> 32) + ": " + cg_error_text(code));
	}
	uint64_t total = 0;
	CL_TRY(cl_scan_u32_u64(ctx, rec_ops.p, op_off.p, n_rec, &total));
	*n_ops = total;
	if (own) { if (total) DEV_ALLOC(ctx, *own, total); d_ops = own->p; cap = total; }
	if (total > cap || (total && !d_ops)) { cl_timing_collect(ctx); return CL_OK; }      // (not filled: the caller refuses)
	if (total)
	{	// (op_off[n_rec] = total <= cap: no operation of the fill lies outside d_ops)
		LAUNCH(ctx, k_cigar_walk<true>, grid, 256, A, d_es, d_es_off, n_reads, limit, CgOut{ d_rec_off, nullptr, rec_ops.p, op_off.p, d_ops }, (unsigned long long*)nullptr);
		HIP_TRY(ctx, hipGetLastError());
		HIP_TRY(ctx, hipStreamSynchronize(cl_launch_stream(ctx)));
	}
	cl_timing_collect(ctx);
	*filled = true;
	return CL_OK;
}
} // namespace

extern "C" cl_status cl_cigars_of(cl_ctx* ctx, const cl_reads* refs, const uint8_t* d_es, const uint64_t* d_es_off, uint32_t n_reads, uint32_t id_limit, uint32_t max_blocks,
                                  uint32_t* d_rec_ops, uint64_t rec_cap, uint64_t* n_rec, uint32_t* d_ops, uint64_t ops_cap, uint64_t* n_ops)
{
	if (n_rec) *n_rec = 0;
	if (n_ops) *n_ops = 0;
	if (!ctx || !refs || !n_rec || !n_ops || (n_reads && (!d_es || !d_es_off))) return cl_fail(ctx, CL_E_INVALID, "cl_cigars_of: null argument");
	if (!n_reads) return CL_OK;
	DevBuf<uint64_t> rec_off; DevBuf<uint32_t> rec_ops;
	uint64_t nr = 0, no = 0; bool filled = false;
	CL_TRY(overlaps_offsets(ctx, "cl_cigars_of", refs, d_es, d_es_off, n_reads, max_blocks, rec_off, &nr));
	// (a capacity that does not hold the operations is 0 to the fill: nothing is written then; nor is anything when the records do not fit)
	const bool rec_fit = nr <= rec_cap && (!nr || d_rec_ops);
	const cl_status s = cg_run(ctx, refs, d_es, d_es_off, n_reads, id_limit ? id_limit : 0xffffffffu, max_blocks, rec_off.p, nr, rec_ops, d_ops, rec_fit ? ops_cap : 0, nullptr, &no, &filled);
	if (s != CL_OK) return s;
	*n_rec = nr; *n_ops = no;
	if (!rec_fit || !filled) return cl_fail(ctx, CL_E_CAPACITY, "cl_cigars_of: need " + std::to_string(nr) + " records and " + std::to_string(no) + " operations");
	if (nr)
	{
		HIP_TRY(ctx, hipMemcpyAsync(d_rec_ops, rec_ops.p, nr * 4, hipMemcpyDeviceToDevice, cl_launch_stream(ctx)));
		HIP_TRY(ctx, hipStreamSynchronize(cl_launch_stream(ctx)));
	}
	return CL_OK;
}

extern "C" cl_status cl_cigars_host(const uint8_t* h_ref_codes, const uint64_t* h_ref_off, uint32_t n_refs, const uint8_t* h_es, const uint64_t* h_es_off, uint64_t n_reads, uint32_t id_limit,
                                    uint32_t* h_rec_ops, uint64_t rec_cap, uint64_t* n_rec, uint32_t* h_ops, uint64_t ops_cap, uint64_t* n_ops, uint64_t* bad_read, uint32_t* bad_code)
{
	if (n_rec) *n_rec = 0;
	if (n_ops) *n_ops = 0;
	if (!n_rec || !n_ops) return CL_E_INVALID;
	std::vector<uint32_t> rec_ops, ops; uint32_t code = 0;
	if (!cg_walk_host(h_ref_codes, h_ref_off, n_refs, h_es, h_es_off, n_reads, id_limit, rec_ops, ops, bad_read, &code))
	{
		if (bad_code) *bad_code = code;
		return code == CGE_RUN ? CL_E_UNSUPPORTED : CL_E_INVALID;
	}
	if (bad_code) *bad_code = 0;
	*n_rec = rec_ops.size(); *n_ops = ops.size();
	if (rec_ops.size() > rec_cap || (!rec_ops.empty() && !h_rec_ops) || ops.size() > ops_cap || (!ops.empty() && !h_ops)) return CL_E_CAPACITY;
	if (!rec_ops.empty()) memcpy(h_rec_ops, rec_ops.data(), rec_ops.size() * 4);
	if (!ops.empty()) memcpy(h_ops, ops.data(), ops.size() * 4);
	return CL_OK;
}
extern "C" const char* cl_cigars_error(uint32_t code) { return cg_error_text(code); }

extern "C" cl_status cl_ctx_set_cigars(cl_ctx* c, int on)
{
	if (!c) return CL_E_INVALID;
	if (on && !c->mappings) return cl_fail(c, CL_E_INVALID, "cl_ctx_set_cigars: needs the mapping records (cl_ctx_set_mappings first)");
	if (on && !c->cigars)
	{	// a new list: this context's and those of the encode lanes a compressor before left on it
		{ std::lock_guard<std::mutex> l(c->cigars_mu); c->cigar_recs.clear(); }
		for (cl_ctx* lane : c->lanes) { std::lock_guard<std::mutex> ll(lane->cigars_mu); lane->cigar_recs.clear(); }
	}
	c->cigars = on != 0;
	if (!on) c->cigars_coded = false;                                          // (the coded form is a form of these)
	return CL_OK;
}
extern "C" cl_status cl_ctx_cigars(const cl_ctx* c, uint32_t* h_rec_ops, uint64_t rec_cap, uint64_t* n_rec, uint32_t* h_ops, uint64_t ops_cap, uint64_t* n_ops)
{
	if (!c || !n_rec || !n_ops) return CL_E_INVALID;
	*n_rec = *n_ops = 0;
	// encode lanes finish out of order: the batches of all of them by their first read
	std::vector<std::pair<uint64_t, const cl_ctx::CigarBatch*>> parts;
	std::vector<std::unique_lock<std::mutex>> locks;
	auto take = [&](const cl_ctx* x) { locks.emplace_back(x->cigars_mu); for (const auto& kv : x->cigar_recs) parts.emplace_back(kv.first, &kv.second); };
	take(c);
	for (const cl_ctx* lane : c->lanes) take(lane);
	std::sort(parts.begin(), parts.end(), [](const auto& a, const auto& b) { return a.first < b.first; });
	uint64_t nr = 0, no = 0;
	for (const auto& p : parts) { nr += p.second->rec_ops.size(); no += p.second->ops.size() + p.second->coded_ops; }
	*n_rec = nr; *n_ops = no;
	if (nr > rec_cap || (nr && !h_rec_ops) || no > ops_cap || (no && !h_ops)) return CL_E_CAPACITY;
	uint64_t ar = 0, ao = 0;
	std::vector<uint32_t> dec;
	for (const auto& p : parts)
	{
		if (!p.second->rec_ops.empty()) memcpy(h_rec_ops + ar, p.second->rec_ops.data(), p.second->rec_ops.size() * 4);
		if (!p.second->ops.empty()) memcpy(h_ops + ao, p.second->ops.data(), p.second->ops.size() * 4);
		if (p.second->coded_ops)
		{	// a batch kept coded (cl_ctx_set_cigars_coded): decoded here, on the host
			dec.clear();
			if (cgc_unpack(p.second->coded.data(), p.second->coded.size(), dec) != CGC_OK || dec.size() != p.second->coded_ops) return CL_E_INVALID;
			memcpy(h_ops + ao, dec.data(), dec.size() * 4);
		}
		ar += p.second->rec_ops.size(); ao += p.second->ops.size() + p.second->coded_ops;
	}
	return CL_OK;
}
extern "C" cl_status cl_compressor_cigars(const cl_compressor* c, uint32_t* h_rec_ops, uint64_t rec_cap, uint64_t* n_rec, uint32_t* h_ops, uint64_t ops_cap, uint64_t* n_ops)
{
	return c ? cl_ctx_cigars(c->ctx, h_rec_ops, rec_cap, n_rec, h_ops, ops_cap, n_ops) : CL_E_INVALID;
}

// Internal (mappings.hip: mappings_chunk): the CIGARs of one batch's records on the genome's pieces.  The counts of the records on other
// references are 0 and hold no operation, so dropping the zeros ON THE HOST — the counts are four bytes per record and come here anyway —
// leaves counts that line up one to one with the lifted records in their stable order, and the operations need no move at all.
cl_status cigars_chunk(cl_ctx* ctx, const cl_reads* refs, const uint8_t* d_es, const uint64_t* d_es_off, uint32_t n_reads, uint64_t first_read, uint32_t id_limit, const uint64_t* d_rec_off,
                       uint64_t n_rec, uint64_t n_lifted)
{
	cl_ctx::CigarBatch B;
	if (n_reads && n_rec)
	{
		DevBuf<uint32_t> rec_ops, ops; uint64_t n_ops = 0; bool filled = false;
		CL_TRY(cg_run(ctx, refs, d_es, d_es_off, n_reads, id_limit, 0, d_rec_off, n_rec, rec_ops, nullptr, 0, &ops, &n_ops, &filled));
		std::vector<uint32_t> all(n_rec);
		const bool coded = ctx->cigars_coded;                                    // the operations stay on the device: their segments come instead (cigar_coder.hip)
		if (coded) { CL_TRY(cigars_pack_device(ctx, "cl_ctx_set_cigars_coded", ops.p, n_ops, 0, 0, B.coded, &B.coded_segments, &B.coded_escapes)); B.coded_ops = n_ops; }
		else B.ops.resize(n_ops);
		HIP_TRY(ctx, hipMemcpyAsync(all.data(), rec_ops.p, n_rec * 4, hipMemcpyDeviceToHost, cl_launch_stream(ctx)));
		if (n_ops && !coded) HIP_TRY(ctx, hipMemcpyAsync(B.ops.data(), ops.p, n_ops * 4, hipMemcpyDeviceToHost, cl_launch_stream(ctx)));
		HIP_TRY(ctx, hipStreamSynchronize(cl_launch_stream(ctx)));
		for (uint32_t c : all) if (c) B.rec_ops.push_back(c);
	}
	if (B.rec_ops.size() != n_lifted) return cl_fail(ctx, CL_E_INVALID, "cl_ctx_set_cigars: " + std::to_string(B.rec_ops.size()) + " CIGARs for " + std::to_string(n_lifted) + " mapping records");
	std::lock_guard<std::mutex> l(ctx->cigars_mu);
	ctx->cigar_recs[first_read] = std::move(B);
	return CL_OK;
}
