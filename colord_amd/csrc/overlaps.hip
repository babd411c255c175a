// overlaps.hip — read-to-read overlaps from the edit scripts on the device (overlaps.hpp): cl_overlaps_of over the tuple
// streams that cl_encode_reads wrote; the host form's C entry; the pipeline's hook (overlaps_chunk) and what a context keeps.
//
// k_overlap_walk<FILL> walks the streams as es_wave.hpp describes: ONE WAVE PER READ, the stream 64 bytes per window (a byte per lane),
// the tuple starts from three ballots, the window cut into stretches on one reference at alt-id / main-ref.  Here, inside a stretch, two
// wave prefix sums — of the cursor advances and of the advances of the READ position — and the open visit's state, which is uniform: a
// stretch's first and last aligned lane come from ctz / clz of `stretch & (match | subst | anchor > 0)`, matches and subst from popcounts
// plus the anchor sum.  It loads no reference base: a position is checked against the reference's length alone (EsRefs<false>: a cursor
// without its word offset).  The tuple that ends a stretch closes the visit; so does the stream's end.
// ONE body, two instantiations, so that the count and the fill cannot disagree: FILL = false writes n_rec[r] and qlen[r]; a prefix sum
// (cl_scan_u32_u64) gives the offsets; FILL = true has lane 0 store the k-th closed visit's record at off[r] + k.
// Persistent blocks of four waves stride over the reads; no LDS, no barrier.
//
// Bounds by construction, in the terms of es_wave.hpp: every loop bound is known before the loop (a window is the
// min(64, bytes left) bytes in front of es_off[r + 1]; the tuple-start loop and the stretch loop run over at most 64 bits of a mask; the
// read loop over n_reads); a window never holds a byte at or past es_off[r + 1] and a tuple that would cross it is an error; every
// reference id is checked against the arena's read count and the translation table's size (OvRefs::A.n is the smaller of the two) before
// lens[] or the table is indexed with it; no reference base is loaded at all.  Stores: n_rec[r] and qlen[r] for r < n_reads; a record only at off[r] + k while
// that is below off[r + 1], and the host has checked off[n_reads] <= cap before the fill is launched.  A malformed stream gives its read
// an error code; the call is CL_E_INVALID and hands nothing out.
#include "common.hpp"
#include "objects.hpp"
#include "es_wave.hpp"
#include "overlaps.hpp"
#include <algorithm>
#include <mutex>

namespace {
// A: lens and n alone, n = the ids that may be met; ref_read: null, or id -> input index (at least A.n entries)
struct OvRefs { Arena A; const uint32_t* ref_read; };

// the open visit closed: a record if it holds an aligned column.  Uniform; lane 0 stores (FILL), three 16-byte vector stores.
template<bool FILL> __device__ inline void ov_close(OvVisit& V, uint32_t& n_rec, const OvRefs& R, const RefCursor& cur, bool is_main, uint32_t q, uint32_t qlen, uint32_t lane,
                                                    cl_overlap* __restrict__ out, uint64_t o0, uint64_t o1)
{
	if (V.has)
	{
		if (FILL && lane == 0 && o0 + n_rec < o1)
		{
			const cl_overlap o = ov_record(V, q, R.ref_read ? R.ref_read[cur.id] : cur.id, qlen, cur.len, cur.rev, is_main);      // (cur.id < A.n: checked where the id was met)
			uint4* dst = reinterpret_cast<uint4*>(out + o0 + n_rec);
			dst[0] = make_uint4(o.q, o.t, o.qlen, o.tlen); dst[1] = make_uint4(o.qs, o.qe, o.ts, o.te); dst[2] = make_uint4(o.matches, o.subst, o.anchor_bases, o.flags);
		}
		++n_rec;
	}
	V = OvVisit();
}

// one read by one wave: the n > 0 stream bytes at s.  Returns the error code (uniform); n_rec = its records, qpos_out = the bases its stream produces.
template<bool FILL> __device__ inline uint32_t ov_read(const OvRefs& R, const uint8_t* __restrict__ s, uint64_t n, uint32_t lane, uint32_t q, uint32_t qlen,
                                                       cl_overlap* __restrict__ out, uint64_t o0, uint64_t o1, uint32_t& n_rec, uint64_t& qpos_out)
{
	uint32_t err = EDE_NONE, lane_err = EDE_NONE;                               // uniform; what a tuple of mine ran into
	const EsStart st = es_start(s, n, lane, R.A.n);
	uint64_t qpos = 0;
	n_rec = 0;
	if (st.plain)
	{	// the rest of the stream is `plain` tuples, a lane per base: no record, the same checks as the profile's
		lane_err = es_plain_check(s, n, lane);
		qpos = n - 1;
	}
	else if (st.err) err = st.err;
	else
	{
		EsRefs<false> F(R.A, st);
		OvVisit V;                                                             // the open visit (uniform)
		uint64_t pos = 5;
		while (!err && pos < n)
		{
			const EsWindow W = es_window(s, pos, n, lane);
			if (W.err) { err = W.err; break; }
			const uint32_t b = W.b, t = W.t, v28 = W.v28; const uint64_t starts = W.starts; const bool is_start = W.is_start;
			// what a tuple advances the reference cursor and the read position by
			const uint32_t adv = es_ref_adv(W), qadv = es_read_adv(W);
			const uint64_t mM = starts & __ballot(t == T_MATCH), mS = starts & __ballot(t == T_SUBST), anch = starts & __ballot(t == T_ANCHOR);
			const uint64_t aligned = mM | mS | (starts & __ballot(t == T_ANCHOR && v28 > 0));
			const uint64_t sw = starts & (W.m5 | __ballot(t == T_MAIN_REF));      // tuples that change the reference
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
					const uint32_t ai = wave_incl_scan(ad), qi = wave_incl_scan(qd);
					const uint32_t atot = __builtin_amdgcn_readfirstlane(__shfl(ai, 63, 64)), qtot = __builtin_amdgcn_readfirstlane(__shfl(qi, 63, 64));
					if (in_seg && (t == T_DEL || t == T_MATCH || t == T_SUBST) && F.cursor + (ai - ad) >= F.cur.len) lane_err = lane_err ? lane_err : (uint32_t)EDE_GUARD;
					uint64_t seg_anchor = 0;
					for (uint64_t am = seg & anch; am; am &= am - 1)
					{	// an anchor: its length, and that it lies on its reference
						const uint32_t l = (uint32_t)__builtin_ctzll(am);
						const uint32_t alen = __builtin_amdgcn_readfirstlane(__shfl(v28, l, 64));
						const uint64_t a_c = F.cursor + (__builtin_amdgcn_readfirstlane(__shfl(ai, l, 64)) - alen);
						if (a_c + alen > F.cur.len) { err = EDE_GUARD; break; }
						seg_anchor += alen;
					}
					if (err) break;
					const uint64_t al = seg & aligned;
					if (al)
					{	// the visit's interval: from in front of its first aligned column to behind its last
						const uint32_t fl = (uint32_t)__builtin_ctzll(al), ll = 63u - (uint32_t)__builtin_clzll(al);
						if (!V.has)
						{
							V.has = true;
							V.qs = qpos + __builtin_amdgcn_readfirstlane(__shfl(qi - qd, fl, 64));
							V.ts_o = F.cursor + __builtin_amdgcn_readfirstlane(__shfl(ai - ad, fl, 64));
						}
						V.qe = qpos + __builtin_amdgcn_readfirstlane(__shfl(qi, ll, 64));
						V.te_o = F.cursor + __builtin_amdgcn_readfirstlane(__shfl(ai, ll, 64));
						V.matches += (uint64_t)__popcll(seg & mM) + seg_anchor; V.subst += (uint64_t)__popcll(seg & mS); V.anchor_bases += seg_anchor;
					}
					F.cursor += atot; qpos += qtot;
				}
				if (sl >= 64) break;
				// the tuple that ends the stretch: a position error inside the visit comes first (the host form meets it first)
				if ((err = es_lane_err(lane < sl ? lane_err : (uint32_t)EDE_NONE))) break;
				// it closes the visit, which lies on the reference left (an alt-id out of range behind it: the read's error, nothing is handed out)
				const bool to_main = __shfl(t, sl, 64) == T_MAIN_REF;
				ov_close<FILL>(V, n_rec, R, F.cur, F.is_main, q, qlen, lane, out, o0, o1);
				if (to_main) F.to_main();
				else if ((err = F.to_alt(R.A, W, sl, lane))) break;
				todo = es_behind(todo, sl);
			}
			if (err) break;
			pos += W.p;
			err = es_lane_err(lane_err);
		}
		if (!err) ov_close<FILL>(V, n_rec, R, F.cur, F.is_main, q, qlen, lane, out, o0, o1);      // the stream's end closes the last visit
	}
	if (!err) err = es_lane_err(lane_err);
	err = __builtin_amdgcn_readfirstlane(err);
	if (!err && qpos > OV_POS_MAX) err = EDE_GUARD;                             // a read position that does not fit the record
	qpos_out = qpos;
	return err;
}

// Blocks stride over quads of reads, one wave each.  FILL = false: n_rec[r], qlen[r] and the first malformed read into *g_err as
// ~(read << 32 | code) (0: none).  FILL = true (after a count without an error): the records of read r at [off[r], off[r + 1]).
template<bool FILL> __global__ __launch_bounds__(256) void k_overlap_walk(OvRefs R, const uint8_t* __restrict__ es, const uint64_t* __restrict__ es_off, uint32_t n_reads, uint32_t first_read,
                                                                          uint32_t* __restrict__ n_rec, uint32_t* __restrict__ qlen, const uint64_t* __restrict__ off,
                                                                          cl_overlap* __restrict__ out, unsigned long long* __restrict__ g_err)
{
	const uint32_t w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6), lane = threadIdx.x & 63;      // (the wave's number is uniform: said so, the read's offsets are scalar loads)
	for (uint64_t r64 = (uint64_t)blockIdx.x * 4 + w; r64 < n_reads; r64 += (uint64_t)gridDim.x * 4)      // (wave-uniform)
	{
		const uint32_t r = (uint32_t)r64;
		const uint64_t a = es_off[r], e = es_off[r + 1], len = e > a ? e - a : 0;
		uint32_t nr = 0; uint64_t qp = 0;
		const uint64_t o0 = FILL ? off[r] : 0, o1 = FILL ? off[r + 1] : 0;
		const uint32_t err = len ? ov_read<FILL>(R, es + a, len, lane, first_read + r, FILL ? qlen[r] : 0u, out, o0, o1, nr, qp) : (uint32_t)EDE_EMPTY;
		if (!FILL && lane == 0)
		{
			n_rec[r] = err ? 0u : nr; qlen[r] = (uint32_t)qp;
			if (err) atomicMax(g_err, ~(((unsigned long long)r << 32) | err));
		}
	}
}

// reference id -> read index: read i of the chunk (input index first + i) is reference bounds[i] iff bounds[i + 1] > bounds[i]
__global__ __launch_bounds__(256) void k_ref_read_scatter(const uint32_t* __restrict__ bounds, uint32_t n, uint32_t first, uint32_t* __restrict__ ref_read, uint32_t n_ref_read)
{
	const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
	if (i >= n) return;
	const uint32_t b = bounds[i];
	if (bounds[i + 1] > b && b < n_ref_read) ref_read[b] = first + (uint32_t)i;
}
} // namespace

// the count: n_rec[r] and qlen[r] of every read, and off = the prefix sum of n_rec (n_reads + 1 entries), *total = off[n_reads].  `who` names
// the entry in the text of a refusal.
static cl_status ov_count(cl_ctx* ctx, const char* who, const OvRefs& R, const uint8_t* d_es, const uint64_t* d_es_off, uint32_t n_reads, uint64_t first_read, uint32_t grid,
                          DevBuf<uint32_t>& n_rec, DevBuf<uint32_t>& qlen, DevBuf<uint64_t>& off, uint64_t* total)
{
	DevBuf<unsigned long long> g;
	DEV_ALLOC(ctx, n_rec, n_reads); DEV_ALLOC(ctx, qlen, n_reads); DEV_ALLOC(ctx, off, (uint64_t)n_reads + 1); DEV_ALLOC(ctx, g, 1);
	HIP_TRY(ctx, hipMemsetAsync(g.p, 0, 8, cl_launch_stream(ctx)));
	LAUNCH(ctx, k_overlap_walk<false>, grid, 256, R, d_es, d_es_off, n_reads, (uint32_t)first_read, n_rec.p, qlen.p, (const uint64_t*)nullptr, (cl_overlap*)nullptr, g.p);
	HIP_TRY(ctx, hipGetLastError());
	unsigned long long h_err = 0;
	HIP_TRY(ctx, hipMemcpyAsync(&h_err, g.p, 8, hipMemcpyDeviceToHost, cl_launch_stream(ctx)));
	HIP_TRY(ctx, hipStreamSynchronize(cl_launch_stream(ctx)));
	if (h_err)
	{
		cl_timing_collect(ctx);
		const uint64_t key = ~(uint64_t)h_err;
		return cl_fail(ctx, CL_E_INVALID, std::string(who) + ": malformed tuple stream, first: read " + std::to_string(key >> 32) + ": " + ed_error_text((uint32_t)key));
	}
	return cl_scan_u32_u64(ctx, n_rec.p, off.p, n_reads, total);
}

// count, place, fill.  The records go to d_out (cap records), or — with `own` — to a buffer made here once the count is known.  off_out (or
// null) takes the records' offsets per read, n_reads + 1 entries.
static cl_status ov_run(cl_ctx* ctx, const cl_reads* refs, const uint8_t* d_es, const uint64_t* d_es_off, uint32_t n_reads, uint64_t first_read, const uint32_t* d_ref_read,
                        uint32_t n_ref_read, uint32_t max_blocks, cl_overlap* d_out, uint64_t cap, DevBuf<cl_overlap>* own, uint64_t* n_out, DevBuf<uint64_t>* off_out = nullptr)
{
	if (n_out) *n_out = 0;
	if (!ctx || !refs || !n_out || (n_reads && (!d_es || !d_es_off)) || (n_ref_read && !d_ref_read)) return cl_fail(ctx, CL_E_INVALID, "cl_overlaps_of: null argument");
	if (first_read + n_reads > OV_POS_MAX + 1) return cl_fail(ctx, CL_E_UNSUPPORTED, "cl_overlaps_of: read indices past 2^32 - 1");
	if (!n_reads) return CL_OK;
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	if (!max_blocks) max_blocks = 4 * (uint32_t)std::max(1, ctx->n_cu);
	const uint32_t grid = std::min(grid_for(n_reads, 4), max_blocks);
	DevBuf<uint32_t> n_rec, qlen; DevBuf<uint64_t> off;
	const OvRefs R{ Arena{ nullptr, nullptr, nullptr, refs->lens.p, d_ref_read ? std::min(refs->n_reads, n_ref_read) : refs->n_reads }, d_ref_read };
	uint64_t total = 0;
	CL_TRY(ov_count(ctx, "cl_overlaps_of", R, d_es, d_es_off, n_reads, first_read, grid, n_rec, qlen, off, &total));
	*n_out = total;
	if (own) { if (total) DEV_ALLOC(ctx, *own, total); d_out = own->p; cap = total; }
	if (total > cap || (total && !d_out)) { cl_timing_collect(ctx); return cl_fail(ctx, CL_E_CAPACITY, "cl_overlaps_of: need " + std::to_string(total) + " records"); }
	if (total)
	{	// (off[n_reads] = total <= cap: no record of the fill lies outside d_out)
		LAUNCH(ctx, k_overlap_walk<true>, grid, 256, R, d_es, d_es_off, n_reads, (uint32_t)first_read, (uint32_t*)nullptr, qlen.p, (const uint64_t*)off.p, d_out, (unsigned long long*)nullptr);
		HIP_TRY(ctx, hipGetLastError());
		HIP_TRY(ctx, hipStreamSynchronize(cl_launch_stream(ctx)));
	}
	cl_timing_collect(ctx);
	if (off_out) *off_out = std::move(off);
	return CL_OK;
}
extern "C" cl_status cl_overlaps_of(cl_ctx* ctx, const cl_reads* refs, const uint8_t* d_es, const uint64_t* d_es_off, uint32_t n_reads, uint64_t first_read,
                                    const uint32_t* d_ref_read, uint32_t n_ref_read, uint32_t max_blocks, cl_overlap* d_out, uint64_t cap, uint64_t* n_out)
{
	return ov_run(ctx, refs, d_es, d_es_off, n_reads, first_read, d_ref_read, n_ref_read, max_blocks, d_out, cap, nullptr, n_out);
}

extern "C" cl_status cl_overlaps_host(const uint8_t* h_ref_codes, const uint64_t* h_ref_off, uint32_t n_refs, const uint8_t* h_es, const uint64_t* h_es_off, uint64_t n_reads,
                                      uint64_t first_read, const uint32_t* h_ref_read, uint32_t n_ref_read, cl_overlap* h_out, uint64_t cap, uint64_t* n_out, uint64_t* bad_read, uint32_t* bad_code)
{
	if (n_out) *n_out = 0;
	if (!n_out) return CL_E_INVALID;
	std::vector<cl_overlap> recs;
	if (!ov_walk_host(h_ref_codes, h_ref_off, n_refs, h_es, h_es_off, n_reads, first_read, h_ref_read, n_ref_read, recs, bad_read, bad_code)) return CL_E_INVALID;
	*n_out = recs.size();
	if (recs.size() > cap || (!recs.empty() && !h_out)) return CL_E_CAPACITY;
	if (!recs.empty()) memcpy(h_out, recs.data(), recs.size() * sizeof(cl_overlap));
	return CL_OK;
}

extern "C" void cl_ctx_set_overlaps(cl_ctx* c, int on)
{
	if (!c) return;
	if (on && !c->overlaps)
	{	// a new list: this context's and those of the encode lanes a compressor before left on it
		{ std::lock_guard<std::mutex> l(c->overlaps_mu); c->overlap_recs.clear(); }
		for (cl_ctx* lane : c->lanes) { std::lock_guard<std::mutex> ll(lane->overlaps_mu); lane->overlap_recs.clear(); }
	}
	c->overlaps = on != 0;
}
extern "C" cl_status cl_ctx_overlaps(const cl_ctx* c, cl_overlap* h_out, uint64_t cap, uint64_t* n_out)
{
	if (!c || !n_out) return CL_E_INVALID;
	*n_out = 0;
	// encode lanes finish out of order: the batches of all of them by their first read
	std::vector<std::pair<uint64_t, const std::vector<cl_overlap>*>> parts;
	std::vector<std::unique_lock<std::mutex>> locks;
	auto take = [&](const cl_ctx* x) { locks.emplace_back(x->overlaps_mu); for (const auto& kv : x->overlap_recs) parts.emplace_back(kv.first, &kv.second); };
	take(c);
	for (const cl_ctx* lane : c->lanes) take(lane);
	std::sort(parts.begin(), parts.end(), [](const auto& a, const auto& b) { return a.first < b.first; });
	uint64_t total = 0;
	for (const auto& p : parts) total += p.second->size();
	*n_out = total;
	if (total > cap || (total && !h_out)) return CL_E_CAPACITY;
	uint64_t at = 0;
	for (const auto& p : parts) { if (!p.second->empty()) memcpy(h_out + at, p.second->data(), p.second->size() * sizeof(cl_overlap)); at += p.second->size(); }
	return CL_OK;
}

// Internal (pass_steps.hpp: tuple_streams): the records of one batch of tuple streams, copied to the host and kept by the context that made them
cl_status overlaps_chunk(cl_ctx* ctx, const cl_reads* refs, const uint8_t* d_es, const uint64_t* d_es_off, uint32_t n_reads, uint64_t first_read, const uint32_t* d_ref_read, uint32_t n_ref_read)
{
	uint64_t n = 0; DevBuf<cl_overlap> out;
	CL_TRY(ov_run(ctx, refs, d_es, d_es_off, n_reads, first_read, d_ref_read, n_ref_read, 0, nullptr, 0, &out, &n));
	std::vector<cl_overlap> h(n);
	if (n)
	{
		HIP_TRY(ctx, hipMemcpyAsync(h.data(), out.p, n * sizeof(cl_overlap), hipMemcpyDeviceToHost, cl_launch_stream(ctx)));
		HIP_TRY(ctx, hipStreamSynchronize(cl_launch_stream(ctx)));
	}
	std::lock_guard<std::mutex> l(ctx->overlaps_mu);
	ctx->overlap_recs[first_read] = std::move(h);
	return CL_OK;
}
// Internal (mappings.hip): the records of one batch with no translation table (`t` is the stream's reference id), in a buffer made here;
// rec_off (or null) takes the records' offsets per read (n_reads + 1 entries), for the walk of cigars.hip
cl_status overlaps_records(cl_ctx* ctx, const cl_reads* refs, const uint8_t* d_es, const uint64_t* d_es_off, uint32_t n_reads, uint64_t first_read, DevBuf<cl_overlap>& out, uint64_t* n_out,
                           DevBuf<uint64_t>* rec_off)
{
	return ov_run(ctx, refs, d_es, d_es_off, n_reads, first_read, nullptr, 0, 0, nullptr, 0, &out, n_out, rec_off);
}
// Internal (cigars.hip): those offsets alone, *n_out = the records: the count of k_overlap_walk and the prefix sum, no fill.  n_reads > 0.
cl_status overlaps_offsets(cl_ctx* ctx, const char* who, const cl_reads* refs, const uint8_t* d_es, const uint64_t* d_es_off, uint32_t n_reads, uint32_t max_blocks, DevBuf<uint64_t>& rec_off,
                           uint64_t* n_out)
{
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	if (!max_blocks) max_blocks = 4 * (uint32_t)std::max(1, ctx->n_cu);
	DevBuf<uint32_t> n_rec, qlen;
	const OvRefs R{ Arena{ nullptr, nullptr, nullptr, refs->lens.p, refs->n_reads }, nullptr };
	return ov_count(ctx, who, R, d_es, d_es_off, n_reads, 0, std::min(grid_for(n_reads, 4), max_blocks), n_rec, qlen, rec_off, n_out);
}
// Internal (stream.hip, driver.hip): the reference id -> read index table of one chunk's `bounds` (n + 1 entries) scattered into d_ref_read
cl_status overlaps_ref_reads(cl_ctx* ctx, const uint32_t* d_bounds, uint32_t n, uint32_t first_read, uint32_t* d_ref_read, uint32_t n_ref_read)
{
	if (!n) return CL_OK;
	LAUNCH(ctx, k_ref_read_scatter, grid_for(n, 256), 256, d_bounds, n, first_read, d_ref_read, n_ref_read);
	HIP_TRY(ctx, hipGetLastError());
	return CL_OK;
}
