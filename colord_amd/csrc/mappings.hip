// mappings.hip — read-to-genome mappings of a reference-genome run on the device (mappings.hpp): cl_mappings_lift over the
// overlap records of a batch (overlaps.hip, no translation table: `t` is the reference id of the stream); the host twin's C entry; the
// pipeline's hook (mappings_chunk) and what a context keeps; the geometry a compressor is given behind its pseudo reads.
//
// k_map_lift<FILL> is a LANE PER RECORD over a grid-stride loop: three 16-byte loads, the target id against n_pseudo, the search in
// piece_first (at most 32 steps, the table is a few entries in cache), three 16-byte stores.  ONE body, two instantiations, so that the
// count and the fill cannot disagree: FILL = false writes keep[i] (1: a record on a genome piece) and the first refused record into
// *g_err; a prefix sum (cl_scan_u32_u64) gives the places, which makes the compaction STABLE: reads stay in input order and a read's
// records in visit order; FILL = true stores the lifted record i at off[i].  No LDS, no barrier, no atomics but the error's.
//
// Bounds by construction: the loop runs over i < n, known before it; record i is read at in + i only; `t` is checked against n_pseudo
// before piece_first is indexed with anything derived from it, and the search stays inside piece_first[0 .. n_seqs] (mappings.hpp);
// seq_len is indexed with s < n_seqs alone.  Stores: keep[i] for i < n; a lifted record only at off[i] for a kept record, and the kept
// records' places are 0 .. total - 1 with total <= cap checked on the host before the fill is launched.  A refused record makes the call
// CL_E_INVALID and hands nothing out.
#include "common.hpp"
#include "objects.hpp"
#include "compressor.hpp"
#include <algorithm>
#include <mutex>

namespace {
template<bool FILL> __global__ __launch_bounds__(256) void k_map_lift(MapGeom G, const cl_overlap* __restrict__ in, uint64_t n, uint32_t* __restrict__ keep, const uint64_t* __restrict__ off,
                                                                      cl_overlap* __restrict__ out, unsigned long long* __restrict__ g_err)
{
	for (uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (uint64_t)gridDim.x * 256)
	{
		const uint4* src = reinterpret_cast<const uint4*>(in + i);
		const uint4 a = src[0], b = src[1], c = src[2];
		const cl_overlap o{ a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w, c.x, c.y, c.z, c.w };
		cl_overlap l = o;
		const bool on_genome = o.t < G.n_pseudo;                              // (before anything is indexed with t)
		const uint32_t err = on_genome ? map_lift_one(G, o, l) : (uint32_t)MAPE_NONE;
		if (!FILL)
		{
			keep[i] = on_genome && !err ? 1u : 0u;
			if (err) atomicMax(g_err, ~(((unsigned long long)i << 32) | err));    // the first refused record: the smallest i is the largest key
		}
		else if (on_genome && !err)
		{
			uint4* dst = reinterpret_cast<uint4*>(out + off[i]);
			dst[0] = make_uint4(l.q, l.t, l.qlen, l.tlen); dst[1] = make_uint4(l.qs, l.qe, l.ts, l.te); dst[2] = make_uint4(l.matches, l.subst, l.anchor_bases, l.flags);
		}
	}
}
} // namespace

// count, place, fill over the n records at d_in with a geometry whose tables are on the device.  The records go to d_out (cap records), or
// — with `own` — to a buffer made here once the count is known.
static cl_status map_run(cl_ctx* ctx, const MapGeom& G, const cl_overlap* d_in, uint64_t n, cl_overlap* d_out, uint64_t cap, DevBuf<cl_overlap>* own, uint64_t* n_out)
{
	*n_out = 0;
	if (n > OV_POS_MAX) return cl_fail(ctx, CL_E_UNSUPPORTED, "cl_mappings_lift: 2^32 records or more in one call");
	if (((uintptr_t)d_in | (uintptr_t)d_out) & 15) return cl_fail(ctx, CL_E_INVALID, "cl_mappings_lift: records must lie at a multiple of 16 bytes");
	if (!n) return CL_OK;
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	const uint32_t grid = std::min(grid_for(n, 256), 8 * (uint32_t)std::max(1, ctx->n_cu));
	DevBuf<uint32_t> keep; DevBuf<uint64_t> off; DevBuf<unsigned long long> g;
	DEV_ALLOC(ctx, keep, n); DEV_ALLOC(ctx, off, n + 1); DEV_ALLOC(ctx, g, 1);
	HIP_TRY(ctx, hipMemsetAsync(g.p, 0, 8, cl_launch_stream(ctx)));
	LAUNCH(ctx, k_map_lift<false>, grid, 256, G, d_in, n, keep.p, (const uint64_t*)nullptr, (cl_overlap*)nullptr, g.p);
	HIP_TRY(ctx, hipGetLastError());
	unsigned long long h_err = 0;
	HIP_TRY(ctx, hipMemcpyAsync(&h_err, g.p, 8, hipMemcpyDeviceToHost, cl_launch_stream(ctx)));
	HIP_TRY(ctx, hipStreamSynchronize(cl_launch_stream(ctx)));
	if (h_err)
	{
		cl_timing_collect(ctx);
		const uint64_t key = ~(uint64_t)h_err;
		return cl_fail(ctx, CL_E_INVALID, "cl_mappings_lift: record " + std::to_string(key >> 32) + ": " + map_error_text((uint32_t)key));
	}
	uint64_t total = 0;
	CL_TRY(cl_scan_u32_u64(ctx, keep.p, off.p, n, &total));
	*n_out = total;
	if (own) { if (total) DEV_ALLOC(ctx, *own, total); d_out = own->p; cap = total; }
	if (total > cap || (total && !d_out)) { cl_timing_collect(ctx); return cl_fail(ctx, CL_E_CAPACITY, "cl_mappings_lift: need " + std::to_string(total) + " records"); }
	if (total)
	{	// (the kept records' places are 0 .. total - 1 and total <= cap: no record of the fill lies outside d_out)
		LAUNCH(ctx, k_map_lift<true>, grid, 256, G, d_in, n, (uint32_t*)nullptr, (const uint64_t*)off.p, d_out, (unsigned long long*)nullptr);
		HIP_TRY(ctx, hipGetLastError());
		HIP_TRY(ctx, hipStreamSynchronize(cl_launch_stream(ctx)));
	}
	cl_timing_collect(ctx);
	return CL_OK;
}

// the tables of a geometry on the device
struct MapTables { DevBuf<uint64_t> seq_len; DevBuf<uint32_t> piece_first; MapGeom G{}; };
static cl_status map_upload(cl_ctx* ctx, const char* who, const uint64_t* h_seq_len, uint32_t n_seqs, uint32_t read_len, uint32_t overlap, std::vector<uint32_t>& pf, MapTables& T)
{
	const cl_status s = map_piece_first(h_seq_len, n_seqs, read_len, overlap, pf);
	if (s == CL_E_UNSUPPORTED) return cl_fail(ctx, s, std::string(who) + ": a sequence of 2^32 bases or more, or 2^32 pieces or more");
	if (s != CL_OK) return cl_fail(ctx, s, std::string(who) + ": the piece length must exceed the overlap, and sequences need their lengths");
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	DEV_ALLOC(ctx, T.seq_len, (uint64_t)n_seqs + 1); DEV_ALLOC(ctx, T.piece_first, (uint64_t)n_seqs + 1);
	if (n_seqs) HIP_TRY(ctx, hipMemcpyAsync(T.seq_len.p, h_seq_len, (uint64_t)n_seqs * 8, hipMemcpyHostToDevice, cl_launch_stream(ctx)));
	HIP_TRY(ctx, hipMemcpyAsync(T.piece_first.p, pf.data(), ((uint64_t)n_seqs + 1) * 4, hipMemcpyHostToDevice, cl_launch_stream(ctx)));
	HIP_TRY(ctx, hipStreamSynchronize(cl_launch_stream(ctx)));
	T.G = MapGeom{ T.seq_len.p, T.piece_first.p, n_seqs, pf[n_seqs], read_len, read_len - overlap };
	return CL_OK;
}

extern "C" cl_status cl_mappings_lift(cl_ctx* ctx, const cl_overlap* d_recs, uint64_t n, const uint64_t* h_seq_len, uint32_t n_seqs, uint32_t read_len, uint32_t overlap,
                                      cl_overlap* d_out, uint64_t cap, uint64_t* n_out)
{
	if (n_out) *n_out = 0;
	if (!ctx || !n_out || (n && !d_recs)) return cl_fail(ctx, CL_E_INVALID, "cl_mappings_lift: null argument");
	std::vector<uint32_t> pf; MapTables T;
	CL_TRY(map_upload(ctx, "cl_mappings_lift", h_seq_len, n_seqs, read_len, overlap, pf, T));
	return map_run(ctx, T.G, d_recs, n, d_out, cap, nullptr, n_out);
}

extern "C" cl_status cl_mappings_lift_host(const cl_overlap* h_recs, uint64_t n, const uint64_t* h_seq_len, uint32_t n_seqs, uint32_t read_len, uint32_t overlap,
                                           cl_overlap* h_out, uint64_t cap, uint64_t* n_out, uint64_t* bad_record, uint32_t* bad_code)
{
	if (n_out) *n_out = 0;
	if (bad_code) *bad_code = 0;
	if (!n_out || (n && !h_recs)) return CL_E_INVALID;
	std::vector<uint32_t> pf;
	CL_TRY(map_piece_first(h_seq_len, n_seqs, read_len, overlap, pf));
	const MapGeom G{ h_seq_len, pf.data(), n_seqs, pf[n_seqs], read_len, read_len - overlap };
	std::vector<cl_overlap> recs;
	if (!map_lift_host(G, h_recs, n, recs, bad_record, bad_code)) return CL_E_INVALID;
	*n_out = recs.size();
	if (recs.size() > cap || (!recs.empty() && !h_out)) return CL_E_CAPACITY;
	if (!recs.empty()) memcpy(h_out, recs.data(), recs.size() * sizeof(cl_overlap));
	return CL_OK;
}

extern "C" void cl_ctx_set_mappings(cl_ctx* c, int on)
{
	if (!c) return;
	if (on && !c->mappings)
	{	// a new list: this context's and those of the encode lanes a compressor before left on it
		{ std::lock_guard<std::mutex> l(c->mappings_mu); c->mapping_recs.clear(); }
		for (cl_ctx* lane : c->lanes) { std::lock_guard<std::mutex> ll(lane->mappings_mu); lane->mapping_recs.clear(); }
	}
	c->mappings = on != 0;
}
extern "C" cl_status cl_ctx_mappings(const cl_ctx* c, cl_overlap* h_out, uint64_t cap, uint64_t* n_out)
{
	if (!c || !n_out) return CL_E_INVALID;
	*n_out = 0;
	// encode lanes finish out of order: the batches of all of them by their first read
	std::vector<std::pair<uint64_t, const std::vector<cl_overlap>*>> parts;
	std::vector<std::unique_lock<std::mutex>> locks;
	auto take = [&](const cl_ctx* x) { locks.emplace_back(x->mappings_mu); for (const auto& kv : x->mapping_recs) parts.emplace_back(kv.first, &kv.second); };
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

// Internal (pass_steps.hpp: tuple_streams): the walk of overlaps.hip over one batch of tuple streams (no table: `t` is the stream's reference
// id), the lift, and the records copied to the host and kept by the context that made them
cl_status mappings_chunk(cl_ctx* ctx, const cl_reads* refs, const uint8_t* d_es, const uint64_t* d_es_off, uint32_t n_reads, uint64_t first_read, const MapGeom* geom)
{
	if (!geom) return cl_fail(ctx, CL_E_INVALID, "cl_ctx_set_mappings: no genome geometry (cl_compressor_genome_geometry)");
	uint64_t n_ov = 0, n = 0; DevBuf<cl_overlap> ov, out; DevBuf<uint64_t> rec_off;
	CL_TRY(overlaps_records(ctx, refs, d_es, d_es_off, n_reads, first_read, ov, &n_ov, ctx->cigars ? &rec_off : nullptr));
	CL_TRY(map_run(ctx, *geom, ov.p, n_ov, nullptr, 0, &out, &n));
	// cl_ctx_set_cigars: the third walk, with the record offsets of this batch's; the records on a piece (id < n_pseudo) are those the lift kept
	if (ctx->cigars) CL_TRY(cigars_chunk(ctx, refs, d_es, d_es_off, n_reads, first_read, geom->n_pseudo, rec_off.p, n_ov, n));
	std::vector<cl_overlap> h(n);
	if (n)
	{
		HIP_TRY(ctx, hipMemcpyAsync(h.data(), out.p, n * sizeof(cl_overlap), hipMemcpyDeviceToHost, cl_launch_stream(ctx)));
		HIP_TRY(ctx, hipStreamSynchronize(cl_launch_stream(ctx)));
	}
	std::lock_guard<std::mutex> l(ctx->mappings_mu);
	ctx->mapping_recs[first_read] = std::move(h);
	return CL_OK;
}

// The geometry of the pseudo reads a compressor was given: the piece count and every piece length are made again from it and must be
// those of the pseudo reads; then the tables stay on the device for the lifts of every batch.
extern "C" cl_status cl_compressor_genome_geometry(cl_compressor* c, const uint64_t* h_seq_len, uint32_t n_seqs, uint32_t read_len, uint32_t overlap)
{
	if (!c) return CL_E_INVALID;
	cl_ctx* ctx = c->ctx;
	if (c->phase != 1 || c->has_map_geom) return cl_fail(ctx, CL_E_INVALID, "cl_compressor_genome_geometry: once, behind cl_compressor_pseudo_reads and before refs_finish");
	std::vector<uint32_t> pf; MapTables T;
	CL_TRY(map_upload(ctx, "cl_compressor_genome_geometry", h_seq_len, n_seqs, read_len, overlap, pf, T));
	if (pf[n_seqs] != c->n_pseudo) return cl_fail(ctx, CL_E_INVALID, "cl_compressor_genome_geometry: the geometry gives " + std::to_string(pf[n_seqs]) + " pieces, the compressor has " + std::to_string(c->n_pseudo) + " pseudo reads");
	if (c->n_pseudo && (c->world == 1 || c->rank == 0))
	{	// (the pseudo reads are the first piece of the reference reads: cl_compressor_pseudo_reads wants to be called before the first refs_add)
		if (c->ref_pieces.empty() || c->ref_pieces[0]->n_reads != c->n_pseudo) return cl_fail(ctx, CL_E_INVALID, "cl_compressor_genome_geometry: the pseudo reads are not at hand");
		std::vector<uint32_t> lens(c->n_pseudo);
		HIP_TRY(ctx, hipMemcpyAsync(lens.data(), c->ref_pieces[0]->lens.p, (uint64_t)c->n_pseudo * 4, hipMemcpyDeviceToHost, cl_launch_stream(ctx)));
		HIP_TRY(ctx, hipStreamSynchronize(cl_launch_stream(ctx)));
		const uint64_t step = read_len - overlap;
		for (uint32_t s = 0; s < n_seqs; ++s)
			for (uint32_t p = pf[s]; p < pf[s + 1]; ++p)
			{
				const uint64_t start = (uint64_t)(p - pf[s]) * step, want = std::min<uint64_t>(read_len, h_seq_len[s] - start);
				if (lens[p] != want) return cl_fail(ctx, CL_E_INVALID, "cl_compressor_genome_geometry: pseudo read " + std::to_string(p) + " has " + std::to_string(lens[p]) + " bases, the geometry gives " + std::to_string(want));
			}
	}
	c->map_seq_len = std::move(T.seq_len); c->map_piece_first = std::move(T.piece_first); c->map_geom = T.G; c->has_map_geom = true;
	c->map_seq_len_h.assign(h_seq_len, h_seq_len + n_seqs);
	return CL_OK;
}
extern "C" cl_status cl_compressor_mappings(const cl_compressor* c, cl_overlap* h_out, uint64_t cap, uint64_t* n_out)
{
	return c ? cl_ctx_mappings(c->ctx, h_out, cap, n_out) : CL_E_INVALID;
}
