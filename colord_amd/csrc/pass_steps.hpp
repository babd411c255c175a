// pass_steps.hpp — the steps of a compression pass that both hosts take, each written once: cl_compress_shard (driver.hip: one call
// over everything) and cl_compressor (stream.hip + lookahead.hip: chunk by chunk) wire the same stages.  What differs stays with the
// callers: their first guesses and regrowth rules for the k-mer scan, and how the index is built (cl_index_build over all lists in one
// call there, cl_index_build_pairs over gathered pairs here — tests/test_gpu_stream.py proves one against the other).  Host code.
#pragma once
#include "common.hpp"
#include "objects.hpp"

static __global__ void k_accept_flags(const uint8_t* __restrict__ acc, const uint8_t* __restrict__ has_n, uint32_t n, uint8_t* __restrict__ out)
{
	const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i < n) out[i] = acc[i] && !has_n[i] ? 1 : 0;
}
template<class T, void (*F)(T*)> struct Handle {      // frees a stage object on scope exit
	T* p = nullptr; ~Handle() { reset(); } void reset() { if (p) F(p); p = nullptr; } T** out() { return &p; } operator T*() const { return p; }
};
template<class T> struct Grow {            // device array that grows geometrically (k-mers of pass 1, index entries of pass 2a)
	DevBuf<T> buf; uint64_t n = 0;
	cl_status reserve(cl_ctx* ctx, uint64_t need)
	{
		if (need <= buf.n) return CL_OK;
		uint64_t cap = std::max<uint64_t>(need, buf.n + buf.n / 2 + 1024);
		DevBuf<T> nb; DEV_ALLOC(ctx, nb, cap);
		if (n) { HIP_TRY(ctx, hipMemcpyAsync(nb.p, buf.p, n * sizeof(T), hipMemcpyDeviceToDevice, ctx->stream)); HIP_TRY(ctx, hipStreamSynchronize(ctx->stream)); }
		buf = std::move(nb);
		return CL_OK;
	}
};

// a1: the k-mers of `reads` behind the g.n that g holds, with room for `want` at first; when the scan finds more, regrow(g, got) says
// how much room the next try gets (the callers' rules differ: they decide allocation sizes, and through the pool, speed)
template<class Regrow> cl_status scan_kmers_into(cl_ctx* ctx, const cl_reads* reads, uint32_t k, uint32_t f, Grow<uint64_t>& g, uint64_t want, Regrow regrow)
{
	for (;;)
	{
		CL_TRY(g.reserve(ctx, g.n + want));
		uint64_t got = 0;
		const cl_status s = cl_kmer_scan(ctx, reads, k, f, g.buf.p + g.n, g.buf.n - g.n, &got);
		if (s == CL_E_CAPACITY) { want = regrow(g, got); continue; }
		CL_TRY(s);
		g.n += got;
		return CL_OK;
	}
}

// host scalars of compression.cpp:443,501-503 over n reads; with a reference genome the counter saw its sequences as reads too and the
// statistics are corrected for them (compression.cpp:443-449).  sparse_range stays 0 without the sparse acceptor.
struct HostScalars { uint64_t mean_read_len = 0; uint32_t sparse_range = 0; };
inline HostScalars host_scalars(const cl_kmer_stats& st, const cl_compress_params& P, uint64_t n, uint64_t genome_seqs, uint64_t genome_len)
{
	HostScalars h;
	if (!n) return h;
	h.mean_read_len = (uint64_t)((double)(st.tot_kmers * P.f) / n + P.k - 1);
	if (genome_seqs)
	{
		const uint64_t n_all = n + genome_seqs;
		const uint64_t m0 = (uint64_t)((double)(st.tot_kmers * P.f) / n_all + P.k - 1);
		h.mean_read_len = (uint64_t)((double)(m0 * n_all - genome_len) / (double)(n_all - genome_seqs));
	}
	if (P.sparse) h.sparse_range = std::max<uint32_t>(1, (uint32_t)((P.sparse_g * (double)st.n_unique_counted * P.f) / (double)(h.mean_read_len ? h.mean_read_len : 1)));
	return h;
}

// a6: the acceptor's one stream over the whole input, n_pseudo pseudo reads in front (ref_reads_accepter.h:41-58); h_accept takes the
// decisions of reads first .. first + n_local.  Without the sparse acceptor it is left as it is (every read accepted).
inline cl_status accept_stream(const cl_compress_params& P, uint32_t n_pseudo, uint64_t n_reads_total, uint32_t range, uint64_t first, uint64_t n_local, uint8_t* h_accept)
{
	if (!P.sparse || !n_reads_total) return CL_OK;
	std::vector<uint8_t> all((size_t)n_pseudo + n_reads_total);
	CL_TRY(cl_ref_accept((uint32_t)n_reads_total, n_pseudo, range, P.sparse_exponent, all.data()));
	std::copy(all.begin() + n_pseudo + first, all.begin() + n_pseudo + first + n_local, h_accept);
	return CL_OK;
}
// ... and on the device: accepted and free of N
inline cl_status accept_flags(cl_ctx* ctx, const uint8_t* h_accept, const cl_reads* reads, DevBuf<uint8_t>& out)
{
	const uint32_t n = reads->n_reads;
	DEV_ALLOC(ctx, out, n);
	DevBuf<uint8_t> d_acc; DEV_ALLOC(ctx, d_acc, n);
	if (n) HIP_TRY(ctx, hipMemcpyAsync(d_acc.p, h_accept, n, hipMemcpyHostToDevice, ctx->stream));
	if (n) LAUNCH(ctx, k_accept_flags, grid_for(n, 256), 256, (const uint8_t*)d_acc.p, (const uint8_t*)reads->has_n.p, n, out.p);
	HIP_TRY(ctx, hipGetLastError());
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	return CL_OK;
}

// index entries of the accepted reads of `lists` (reference ids from ref_base on) behind those that pair_ids / pair_refs hold
inline cl_status append_index_entries(cl_ctx* ctx, const cl_kmer_lists* lists, const uint8_t* d_accept, uint32_t ref_base, Grow<uint32_t>& pair_ids, Grow<uint32_t>& pair_refs)
{
	uint64_t n_sel = 0;
	const cl_status s = cl_index_entries_of(ctx, lists, d_accept, ref_base, nullptr, nullptr, 0, &n_sel, nullptr, nullptr);
	if (s != CL_OK && s != CL_E_CAPACITY) return s;
	if (!n_sel) return CL_OK;
	CL_TRY(pair_ids.reserve(ctx, pair_ids.n + n_sel)); CL_TRY(pair_refs.reserve(ctx, pair_refs.n + n_sel));
	CL_TRY(cl_index_entries_of(ctx, lists, d_accept, ref_base, pair_ids.buf.p + pair_ids.n, pair_refs.buf.p + pair_refs.n, n_sel, &n_sel, nullptr, nullptr));
	pair_ids.n += n_sel; pair_refs.n += n_sel;
	return CL_OK;
}

// Stage A of a batch of reads on context `ctx` (the caller's, or an encode lane's): from their accepted k-mers (a4: `lists`, released
// here as soon as they have served) a5 candidates among the reference reads before each read (d_bounds), a8/a9 anchors, a10-a12 edit
// scripts -> tuple streams.  Reads only state that is complete (index, reference reads), so batches are independent here.
struct TupleStreams { DevBuf<uint8_t> es; DevBuf<uint64_t> es_off; DevBuf<uint32_t> es_nt; uint64_t es_bytes = 0, n_anchors = 0; };
// cl_ctx_set_verify: every read of the batch rebuilt on the device from its edit script and the reference reads (expand.hip, the inverse
// of a10-a12) and compared with the input, before anything is coded from the streams.  The entropy-coded bytes are not covered.
inline cl_status verify_streams(cl_ctx* ctx, const cl_reads* reads, const cl_reads* refs, const TupleStreams& ts)
{
	uint64_t n_bad = 0; uint32_t first_bad = 0, first_diff = 0;
	CL_TRY(cl_es_verify_at(ctx, reads, refs, ts.es.p, ts.es_off.p, ts.es_nt.p, ts.es_bytes, &n_bad, &first_bad, &first_diff));
	if (n_bad)
		return cl_fail(ctx, CL_E_MISMATCH, "edit-script check: " + std::to_string(n_bad) + " of " + std::to_string(reads->n_reads) + " reads are not rebuilt from their edit scripts; first: read " +
			std::to_string(first_bad) + " of the chunk, " + (first_diff == 0xffffffffu ? std::string("its length or tuple count differs") : "first differing base " + std::to_string(first_diff)));
	ctx->verified_reads += reads->n_reads; ctx->verified_bases += reads->total_bases;
	return CL_OK;
}
inline cl_status tuple_streams(cl_ctx* ctx, const cl_compress_params* P, Handle<cl_kmer_lists, cl_kmer_lists_free>& lists, const cl_index* index, const cl_reads* refs,
                               const cl_reads* reads, const uint32_t* d_bounds, const uint32_t* h_pack_bounds, uint32_t n_packs, uint64_t first_read, const uint32_t* d_ref_read,
                               uint32_t n_ref_read, const MapGeom* map_geom, cl_pileup* pileup, TupleStreams& out)
{
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	const uint32_t n = reads->n_reads;
	// more than 16 candidates per read / more than 8 recursion levels (the reference takes any value; its presets stop at 12 and 6): this
	// build's frames hold 16 candidate views and 10 levels — the read is coded against its 16 best candidates, to depth 8.  Still a
	// valid archive (the alternative-id model keeps the alphabet of P->c symbols the `meta` stream announces), a little larger than
	// the reference's would be; never a failed call.
	const uint32_t cc = std::min<uint32_t>(P->c, 16), max_rec = std::min<uint32_t>(P->max_rec, 8);
	DevBuf<uint32_t> crefs, votes, cnt; DEV_ALLOC(ctx, crefs, (uint64_t)n * cc); DEV_ALLOC(ctx, votes, (uint64_t)n * cc); DEV_ALLOC(ctx, cnt, n);
	CL_TRY(cl_candidates_at(ctx, index, lists, d_bounds, cc, crefs.p, votes.p, cnt.p));
	votes.release();
	DevBuf<uint64_t> common_off, common;
	const bool hifi = P->source == 2;
	if (hifi)
	{
		DEV_ALLOC(ctx, common_off, (uint64_t)n * cc + 1);
		uint64_t need = 0;
		cl_status s = cl_candidates_common(ctx, index, lists, cc, crefs.p, cnt.p, common_off.p, nullptr, 0, &need);
		if (s != CL_OK && s != CL_E_CAPACITY) return s;
		DEV_ALLOC(ctx, common, need + 1);
		CL_TRY(cl_candidates_common(ctx, index, lists, cc, crefs.p, cnt.p, common_off.p, common.p, need, &need));
	}
	lists.reset();
	Handle<cl_anchors, cl_anchors_free> anc;
	CL_TRY(cl_anchor_candidates_hifi(ctx, reads, refs, crefs.p, cnt.p, cc, P->anchor_len, P->frac_always, P->frac_min, P->max_matches_mult, P->min_anchors,
		P->k, P->f, hifi ? common_off.p : nullptr, hifi ? common.p : nullptr, anc.out()));
	out.n_anchors = cl_anchors_total(anc);
	crefs.release(); cnt.release(); common_off.release(); common.release();
	const uint64_t es_cap = reads->total_bases + 16ull * n + 4096;
	DEV_ALLOC(ctx, out.es, es_cap); DEV_ALLOC(ctx, out.es_off, (uint64_t)n + 1); DEV_ALLOC(ctx, out.es_nt, n);
	CL_TRY(cl_encode_reads(ctx, reads, refs, anc, cc, P->anchor_len, P->min_part_alt, max_rec, P->cost_mult, h_pack_bounds, n_packs, out.es.p, es_cap, out.es_off.p, out.es_nt.p, &out.es_bytes));
	if (ctx->verify) CL_TRY(verify_streams(ctx, reads, refs, out));
	if (ctx->edit_profile) CL_TRY(edit_profile_chunk(ctx, refs, out.es.p, out.es_off.p, n));
	// cl_ctx_set_overlaps: the batch's first read is read `first_read` of the input; d_ref_read: reference id -> input index (overlaps.hip)
	if (ctx->overlaps) CL_TRY(overlaps_chunk(ctx, refs, out.es.p, out.es_off.p, n, first_read, d_ref_read, n_ref_read));
	// cl_ctx_set_mappings: the same walk with the ids as they are, then the lift to the genome's sequences (mappings.hip)
	if (ctx->mappings) CL_TRY(mappings_chunk(ctx, refs, out.es.p, out.es_off.p, n, first_read, map_geom));
	// cl_ctx_set_pileup: the walk once more, every tuple on a genome piece booked at its genome position in the compressor's table (pileup.hip)
	return ctx->pileup ? pileup_chunk(ctx, pileup, refs, out.es.p, out.es_off.p, n) : CL_OK;
}

// The coder tail of a batch: a14 + a16 the DNA stream, a13 + a15 the quality stream.  The quality stream of level 1 does not depend on
// the edit scripts: when its coder lives on a second context of the same GPU (own stream, own pool), start_quality() codes it on a
// thread of its own beside whatever the caller does until code() — both are latency-bound chains that leave most of the machine idle.
// Otherwise code() takes it after the DNA stream on the same context (levels 2 and 3: with the per-base classes of the scripts).
struct ChunkIO {
	const cl_reads* reads; const uint8_t* d_quals; const uint64_t* d_base_off; const uint32_t* h_part_bounds; uint32_t n_parts;
	uint8_t* d_dna_out; uint64_t dna_cap; uint64_t* h_dna_part_sizes; uint8_t* d_qual_out; uint64_t qual_cap; uint64_t* h_qual_part_sizes; cl_compress_info* info;
};
struct ChunkCoder {
	cl_ctx* ctx; uint32_t level; cl_dna_coder* dna; cl_qual_coder* qual; ChunkIO io;
	cl_ctx* qctx; bool overlap; std::thread qthread; cl_status qstatus = CL_OK;
	ChunkCoder(cl_ctx* c, uint32_t lvl, cl_dna_coder* d, cl_qual_coder* q, const ChunkIO& io_)
		: ctx(c), level(lvl), dna(d), qual(q), io(io_), qctx(q ? cl_qual_coder_ctx(q) : nullptr), overlap(q && lvl <= 1 && qctx && qctx != c) {}
	~ChunkCoder() { if (qthread.joinable()) qthread.join(); }
	cl_status quality_on(cl_ctx* on, const uint8_t* d_flags)
	{
		if (on != ctx) on->verify_streams = ctx->verify_streams;      // (the quality coder's own context checks its parts when the caller's does)
		return cl_qual_encode(on, qual, io.reads, io.d_quals, io.d_base_off, d_flags, io.h_part_bounds, io.n_parts, io.d_qual_out, io.qual_cap, io.h_qual_part_sizes, &io.info->qual_bytes);
	}
	void start_quality() { if (overlap) qthread = std::thread([this]() { qstatus = quality_on(qctx, nullptr); }); }
	cl_status code(const cl_reads* refs, const TupleStreams& ts)
	{
		CL_TRY(cl_dna_encode(ctx, dna, refs, ts.es.p, ts.es_off.p, ts.es_nt.p, io.reads->n_reads, io.h_part_bounds, io.n_parts, io.d_dna_out, io.dna_cap, io.h_dna_part_sizes, &io.info->dna_bytes));
		if (overlap)
		{
			qthread.join();
			return qstatus == CL_OK ? CL_OK : cl_fail(ctx, qstatus, std::string("quality stream: ") + cl_last_error(qctx));
		}
		if (!qual) return CL_OK;
		DevBuf<uint8_t> flags;
		if (level > 1)
		{
			DEV_ALLOC(ctx, flags, io.reads->total_bases + 1);
			CL_TRY(cl_es_flags(ctx, io.reads, ts.es.p, ts.es_off.p, io.d_base_off, flags.p));
		}
		return quality_on(ctx, level > 1 ? flags.p : nullptr);
	}
};

// kernel times of a worker's context added to another's, every field (`cells` is set by the aligner launches of encode_es.hip only:
// the maps of the preparation contexts carry zero there)
inline void merge_times(std::map<std::string, KernelTime>& dst, const std::map<std::string, KernelTime>& src)
{
	for (auto& kv : src) { auto& t = dst[kv.first]; t.ms += kv.second.ms; t.launches += kv.second.launches; t.bytes += kv.second.bytes; t.cells += kv.second.cells; }
}
