// driver.hip — the compress data path of one shard as ONE native call: what runCompression wires together with threads
// and queues (src/colord/compression.cpp:432-689: CKmerCounter -> CKmerFilter -> CRefReadsAccepter ->
// CReadsSimilarityGraph -> CEncoder -> CEntrComprReads / CEntrComprQuals), here a straight sequence of the stage entry
// points of this library on one GPU stream.  Host code only; every byte of the result comes from the HIP stages.
#include "pass_steps.hpp"
extern "C" cl_status cl_compress_shard(cl_ctx* ctx, const cl_compress_params* P, const cl_reads* reads, const uint8_t* d_quals, const uint64_t* d_base_off,
                                       const uint32_t* h_part_bounds, uint32_t n_parts, const uint32_t* h_pack_bounds, uint32_t n_packs,
                                       cl_dna_coder* dna, cl_qual_coder* qual,
                                       uint8_t* d_dna_out, uint64_t dna_cap, uint64_t* h_dna_part_sizes,
                                       uint8_t* d_qual_out, uint64_t qual_cap, uint64_t* h_qual_part_sizes, cl_compress_info* info)
{
	if (!ctx || !P || !reads || !h_part_bounds || !h_pack_bounds || !dna || !info) return cl_fail(ctx, CL_E_INVALID, "cl_compress_shard: null argument");
	if (qual && (!d_quals || !d_base_off || !h_qual_part_sizes)) return cl_fail(ctx, CL_E_INVALID, "cl_compress_shard: quality coder without qualities");
	if (ctx->mappings) return cl_fail(ctx, CL_E_UNSUPPORTED, "cl_compress_shard: cl_ctx_set_mappings needs the pseudo reads of a reference genome, which one shard does not have (cl_compressor)");
	if (ctx->cigars) return cl_fail(ctx, CL_E_UNSUPPORTED, "cl_compress_shard: cl_ctx_set_cigars needs the mapping records of a reference genome, which one shard does not have (cl_compressor)");
	if (ctx->pileup) return cl_fail(ctx, CL_E_UNSUPPORTED, "cl_compress_shard: cl_ctx_set_pileup needs the pseudo reads of a reference genome, which one shard does not have (cl_compressor)");
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	memset(info, 0, sizeof(*info));
	const uint32_t n = reads->n_reads;
	info->n_reads = n; info->n_bases = reads->total_bases;
	if (!n) return CL_OK;
	if (ctx->digest) CL_TRY(digest_chunk(ctx, reads, cl_qual_coder_params(qual), d_quals, d_base_off, 0));     // from the input, before anything is made of it
	if (ctx->digest_values) CL_TRY(digest_values_chunk(ctx, reads, cl_qual_coder_params(qual), d_quals, d_base_off, 0));
	if (ctx->report) CL_TRY(report_chunk(ctx, reads, cl_qual_coder_params(qual), d_quals, d_base_off));
	// the quality stream beside the whole DNA path where it may be (level 1, a context of its own)
	ChunkCoder coder(ctx, P->level, dna, qual, ChunkIO{ reads, d_quals, d_base_off, h_part_bounds, n_parts, d_dna_out, dna_cap, h_dna_part_sizes, d_qual_out, qual_cap, h_qual_part_sizes, info });
	coder.start_quality();
	// a1 + a2 + a3: k-mer scan, exact count / threshold, membership set (compression.cpp:432-464)
	Handle<cl_kmer_set, cl_kmer_set_free> kset; cl_kmer_stats ks{};
	{
		const uint64_t cap = P->f > 1 ? (uint64_t)(reads->total_bases / P->f * 1.3) + 4096 : reads->total_bases + 64;
		Grow<uint64_t> km; DEV_ALLOC(ctx, km.buf, cap);
		CL_TRY(scan_kmers_into(ctx, reads, P->k, P->f, km, cap, [](Grow<uint64_t>& g, uint64_t got) { g.buf.release(); return got; }));    // (a second try: exactly what the first one found)
		CL_TRY(cl_kmer_count_filter(ctx, km.buf.p, km.n, P->k, P->ci, P->cs, kset.out(), &ks));
	}
	info->tot_kmers = ks.tot_kmers; info->n_kept_kmers = ks.n_unique_counted;
	// a4: accepted k-mers per read
	Handle<cl_kmer_lists, cl_kmer_lists_free> lists;
	CL_TRY(cl_accepted_kmers(ctx, kset, reads, P->k, P->f, lists.out()));
	// a6: acceptor
	info->sparse_range = host_scalars(ks, *P, n, 0, 0).sparse_range;
	std::vector<uint8_t> h_acc(n, 1);
	CL_TRY(accept_stream(*P, 0, n, info->sparse_range, 0, n, h_acc.data()));
	DevBuf<uint8_t> accept;
	CL_TRY(accept_flags(ctx, h_acc.data(), reads, accept));
	// a5: index over all lists in one call; a7: reference reads
	Handle<cl_index, cl_index_free> index;
	CL_TRY(cl_index_build(ctx, kset, lists, accept.p, 0, P->cs, index.out()));
	Handle<cl_reads, cl_reads_free> refs;
	CL_TRY(cl_reads_select(ctx, reads, accept.p, refs.out()));
	info->n_refs = refs.p->n_reads;
	// a5 candidates (every read against the reference reads before it: the index's own ranks) ... a12 tuple streams; then the coders
	TupleStreams ts;
	DevBuf<uint32_t> ref_read;                                 // cl_ctx_set_overlaps: reference id -> read index of this one shard, from the index's ranks
	if (ctx->overlaps && refs.p->n_reads)
	{
		DEV_ALLOC(ctx, ref_read, refs.p->n_reads);
		HIP_TRY(ctx, hipMemsetAsync(ref_read.p, 0xff, (uint64_t)refs.p->n_reads * 4, cl_launch_stream(ctx)));
		CL_TRY(overlaps_ref_reads(ctx, cl_index_ref_rank(index), n, 0, ref_read.p, refs.p->n_reads));
	}
	CL_TRY(tuple_streams(ctx, P, lists, index, refs, reads, cl_index_ref_rank(index), h_pack_bounds, n_packs, 0, ref_read.p, ref_read.p ? refs.p->n_reads : 0u, nullptr, nullptr, ts));
	info->n_anchors = ts.n_anchors; info->tuple_bytes = ts.es_bytes;
	return coder.code(refs, ts);
}
