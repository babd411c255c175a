// stream.hip — runCompression for inputs that do not fit one call, and for reads sharded over GPUs.
//
// The reference streams a file of any size through its two passes: pass 1 counts the k-mers of the WHOLE input
// (compression.cpp:432, CKmerCounter), pass 2 pushes reader packs of 4 Mi symbols through graph -> encoder -> coders
// (compression.cpp:547-561, in_reads.cpp:62-77), the similarity graph growing as reference reads pass by
// (reads_sim_graph.cpp:324-427).  cl_compressor is that state between calls; the caller hands it the input CHUNK by
// chunk (a chunk = whole reader packs, e.g. 1 Gbase), three times:
//   count_add*  -> count_finish      pass 1: surviving k-mers accumulate, then exact counts / the filtered set
//   refs_add*   -> refs_finish       which reads become reference reads (acceptor), their store (a7) and the k-mer ->
//                                    reference-reads index over the whole input; a read of any chunk sees exactly the
//                                    index entries of EARLIER reference reads (lists are prefixes in id order, SURVEY
//                                    App. F1), so the chunked result is byte-identical to one call over everything
//   encode*                          pass 2: candidates, anchors, edit scripts, `dna` / `qual` parts of a chunk; the
//                                    coders' adaptive models persist from chunk to chunk as in one CEntrCompr* thread
// With a cl_exchange (one process per GPU, reads sharded in file order) the two finish steps run the exchanges of SURVEY
// §8e: k-mers to the owner of their key range, kept keys all-gathered (replicated set); reference reads and index
// entries all-gathered (replicated store + index).  The collectives themselves are the caller's (torch.distributed over
// RCCL in colord_amd/parallel.py); this file only says what is exchanged.  The steps it shares with cl_compress_shard are in
// pass_steps.hpp, the state in compressor.hpp, the look-ahead of pass 2b in lookahead.hip.  Host code; all data work is in the stages.
#include "compressor.hpp"

namespace {
__global__ void k_add_u32(uint32_t* v, uint64_t n, uint32_t c) { const uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; if (i < n) v[i] += c; }
// k-mers grouped by destination rank (the owner of the 4096-bin range a key falls into); cursor[r] = start of r's group
__global__ __launch_bounds__(256) void k_owner_scatter(const uint64_t* __restrict__ keys, uint64_t n, uint32_t shift, const uint32_t* __restrict__ owner_of_bin,
                                                       uint32_t world, unsigned long long* __restrict__ cursor, uint64_t* __restrict__ out)
{
	__shared__ uint32_t cnt[64];
	__shared__ unsigned long long base[64];
	if (threadIdx.x < 64) cnt[threadIdx.x] = 0;
	__syncthreads();
	const uint64_t i = (uint64_t)blockIdx.x * 256 + threadIdx.x;
	uint64_t key = 0; uint32_t o = 0, my = 0;
	if (i < n) { key = keys[i]; o = owner_of_bin[(uint32_t)(key >> shift) & 4095u]; my = atomicAdd(&cnt[o], 1u); }
	__syncthreads();
	if (threadIdx.x < world && cnt[threadIdx.x]) base[threadIdx.x] = atomicAdd(&cursor[threadIdx.x], (unsigned long long)cnt[threadIdx.x]);
	__syncthreads();
	if (i < n) out[base[o] + my] = key;
}
} // namespace

cl_compressor::~cl_compressor()
{
	la.stop();
	if (getenv("COLORD_HIP_STREAM_DEBUG")) la.report(enc_chunk);
	for (auto* r : ref_pieces) cl_reads_free(r);
	if (pileup) cl_pileup_free(pileup);
	if (refs) cl_reads_free(refs);
	if (index) cl_index_free(index);
	if (kset) cl_kmer_set_free(kset);
	if (dna) cl_dna_coder_free(dna);
	if (qual) cl_qual_coder_free(qual);
}

extern "C" cl_status cl_compressor_create(cl_ctx* ctx, cl_ctx* qual_ctx, const cl_compress_params* params, const cl_qual_params* qparams,
                                          const cl_exchange* exchange, uint64_t expected_bases, cl_compressor** out)
{
	if (!ctx || !params || !out) return cl_fail(ctx, CL_E_INVALID, "cl_compressor_create: null argument");
	if (exchange && (exchange->world < 1 || exchange->world > 64 || exchange->rank >= exchange->world ||
	                 (exchange->world > 1 && (!exchange->all_gather_host || !exchange->all_to_all_v || !exchange->all_gather_v))))
		return cl_fail(ctx, CL_E_INVALID, "cl_compressor_create: exchange needs 1 <= world <= 64, rank < world and its three collectives");
	cl_compressor* c = new cl_compressor();
	c->ctx = ctx; c->qctx = qual_ctx ? qual_ctx : ctx; c->P = *params; c->expected_bases = expected_bases;
	if (qparams) { c->has_qual = true; c->Q = *qparams; }
	if (exchange && exchange->world > 1) { c->X = *exchange; c->rank = exchange->rank; c->world = exchange->world; }
	if (cl_cu_mask_cfg().any || getenv("COLORD_HIP_ROLE_PRIO"))
	{	// CU partitioning (COLORD_HIP_CU_MASK) / priorities by role: the caller's two contexts take their roles' CUs (their streams are made anew, idle as they are)
		cl_ctx_set_priority(ctx, 0, CL_ROLE_MAIN);
		if (qual_ctx && qual_ctx != ctx) cl_ctx_set_priority(qual_ctx, 0, CL_ROLE_QUAL);
	}
	*out = c;
	return CL_OK;
}
extern "C" void cl_compressor_free(cl_compressor* c) { delete c; }

// ---- pass 1 ---------------------------------------------------------------------------------------------------------
// room for the k-mers of an input at first, and after a scan that found `got`
static uint64_t first_guess(const cl_reads* r, uint32_t f) { return f > 1 ? (uint64_t)(r->total_bases / f * 1.15) + 4096 : r->total_bases + 64; }
static uint64_t regrow(Grow<uint64_t>&, uint64_t got) { return got + got / 64; }

extern "C" cl_status cl_compressor_count_add(cl_compressor* c, const cl_reads* chunk)
{
	if (!c || !chunk) return CL_E_INVALID;
	cl_ctx* ctx = c->ctx;
	if (c->phase != 0) return cl_fail(ctx, CL_E_INVALID, "cl_compressor_count_add: pass 1 is already finished");
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	const uint32_t f = c->P.f;
	uint64_t want = first_guess(chunk, f);
	if (!c->kmers.buf.n && c->expected_bases > chunk->total_bases)          // one allocation for the whole input when its size is known
		CL_TRY(c->kmers.reserve(ctx, f > 1 ? (uint64_t)(c->expected_bases / f * 1.03) + 4096 : c->expected_bases + 64));
	if (c->kmers.buf.n - c->kmers.n >= chunk->total_bases / f) want = c->kmers.buf.n - c->kmers.n;     // what is left probably holds the chunk: no regrowth
	CL_TRY(scan_kmers_into(ctx, chunk, c->P.k, f, c->kmers, want, regrow));
	c->chunk_reads.push_back(chunk->n_reads);
	c->n_reads_local += chunk->n_reads; c->n_bases_local += chunk->total_bases;
	return CL_OK;
}

// Reference-genome mode, pass 1 (compression.cpp:405-429): the genome's sequences are a second input of the k-mer counter.
extern "C" cl_status cl_compressor_genome_add(cl_compressor* c, const cl_reads* seqs)
{
	if (!c || !seqs) return CL_E_INVALID;
	cl_ctx* ctx = c->ctx;
	if (c->phase != 0) return cl_fail(ctx, CL_E_INVALID, "cl_compressor_genome_add: pass 1 is already finished");
	// Sharded reads: every rank is given the same sequences; rank 0 alone scans them (the k-mers travel to their owners with
	// the rest in count_finish), the others only note the numbers the statistics are corrected by.
	if (c->world > 1 && c->rank != 0) { c->genome_seqs += seqs->n_reads; c->genome_len += seqs->total_bases; return CL_OK; }
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	CL_TRY(scan_kmers_into(ctx, seqs, c->P.k, c->P.f, c->kmers, first_guess(seqs, c->P.f), regrow));
	c->genome_seqs += seqs->n_reads; c->genome_len += seqs->total_bases;
	return CL_OK;
}

// k-mers to the rank that owns their key range; returns the received k-mers in c->kmers
static cl_status exchange_kmers(cl_compressor* c)
{
	cl_ctx* ctx = c->ctx; const uint32_t W = c->world, k = c->P.k;
	std::vector<uint64_t> bins;
	CL_TRY(cl_key_histogram(ctx, c->kmers.buf.p, c->kmers.n, k, bins));
	// global histogram -> W contiguous bin ranges of about equal weight (the same cut on every rank)
	std::vector<uint64_t> all((size_t)W * 4096);
	CL_TRY(c->X.all_gather_host(c->X.user, bins.data(), 4096, all.data()));
	std::vector<uint64_t> g(4096, 0); uint64_t total = 0;
	for (uint32_t r = 0; r < W; ++r) for (uint32_t b = 0; b < 4096; ++b) g[b] += all[(size_t)r * 4096 + b];
	for (uint64_t v : g) total += v;
	std::vector<uint32_t> owner(4096); uint64_t acc = 0; uint32_t r = 0;
	for (uint32_t b = 0; b < 4096; ++b)
	{
		while (r + 1 < W && acc >= (total * (r + 1) + W - 1) / W) ++r;
		owner[b] = r; acc += g[b];
	}
	DevBuf<uint32_t> d_owner; DEV_ALLOC(ctx, d_owner, 4096);
	HIP_TRY(ctx, hipMemcpyAsync(d_owner.p, owner.data(), 4096 * 4, hipMemcpyHostToDevice, ctx->stream));
	std::vector<uint64_t> send(W, 0);
	for (uint32_t b = 0; b < 4096; ++b) send[owner[b]] += bins[b];
	std::vector<unsigned long long> cur(W, 0);
	for (uint32_t i = 1; i < W; ++i) cur[i] = cur[i - 1] + send[i - 1];
	DevBuf<unsigned long long> d_cur; DEV_ALLOC(ctx, d_cur, 64);
	HIP_TRY(ctx, hipMemcpyAsync(d_cur.p, cur.data(), W * 8, hipMemcpyHostToDevice, ctx->stream));
	DevBuf<uint64_t> sorted; DEV_ALLOC(ctx, sorted, c->kmers.n);
	if (c->kmers.n)
		LAUNCHB(ctx, c->kmers.n * 16.0, k_owner_scatter, grid_for(c->kmers.n, 256), 256, (const uint64_t*)c->kmers.buf.p, c->kmers.n, cl_part_shift(k), (const uint32_t*)d_owner.p, W, d_cur.p, sorted.p);
	HIP_TRY(ctx, hipGetLastError());
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	// counts each rank sends to me
	std::vector<uint64_t> mat((size_t)W * W);
	CL_TRY(c->X.all_gather_host(c->X.user, send.data(), W, mat.data()));
	std::vector<uint64_t> sb(W), rb(W); uint64_t n_recv = 0;
	for (uint32_t i = 0; i < W; ++i) { sb[i] = send[i] * 8; rb[i] = mat[(size_t)i * W + c->rank] * 8; n_recv += mat[(size_t)i * W + c->rank]; }
	c->kmers.buf.release(); c->kmers.n = 0;
	DevBuf<uint64_t> recv; DEV_ALLOC(ctx, recv, n_recv);
	CL_TRY(c->X.all_to_all_v(c->X.user, sorted.p, sb.data(), recv.p, rb.data()));
	c->kmers.buf = std::move(recv); c->kmers.n = n_recv;
	return CL_OK;
}

extern "C" cl_status cl_compressor_count_finish(cl_compressor* c, cl_kmer_stats* stats)
{
	if (!c) return CL_E_INVALID;
	cl_ctx* ctx = c->ctx;
	if (c->phase != 0) return cl_fail(ctx, CL_E_INVALID, "cl_compressor_count_finish: called twice");
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	const uint32_t W = c->world;
	cl_kmer_stats st{};
	if (W > 1) CL_TRY(exchange_kmers(c));
	CL_TRY(cl_kmer_count_filter(ctx, c->kmers.buf.p, c->kmers.n, c->P.k, c->P.ci, c->P.cs, &c->kset, &st));
	c->kmers.buf.release(); c->kmers.n = 0;
	c->first_read = 0; c->n_reads_total = c->n_reads_local;
	if (W > 1)
	{
		// replicate the filtered set: partitions are key ranges in rank order, so the concatenation is ascending
		uint64_t mine[6] = { st.tot_kmers, st.n_unique, st.n_unique_counted, st.total_count_filtered, c->n_reads_local, 0 };
		std::vector<uint64_t> all((size_t)W * 6);
		CL_TRY(c->X.all_gather_host(c->X.user, mine, 6, all.data()));
		std::vector<uint64_t> kb(W), cb(W); uint64_t n_all = 0;
		st = cl_kmer_stats{}; c->n_reads_total = 0;
		for (uint32_t r = 0; r < W; ++r)
		{
			const uint64_t* a = &all[(size_t)r * 6];
			st.tot_kmers += a[0]; st.n_unique += a[1]; st.n_unique_counted += a[2]; st.total_count_filtered += a[3];
			if (r < c->rank) c->first_read += a[4];
			c->n_reads_total += a[4];
			kb[r] = a[2] * 8; cb[r] = a[2] * 4; n_all += a[2];
		}
		if (n_all >= (1ull << 32)) return cl_fail(ctx, CL_E_UNSUPPORTED, "cl_compressor_count_finish: >= 2^32 kept k-mers");
		DevBuf<uint64_t> keys; DevBuf<uint32_t> counts; DEV_ALLOC(ctx, keys, n_all); DEV_ALLOC(ctx, counts, n_all);
		CL_TRY(c->X.all_gather_v(c->X.user, cl_kmer_set_keys(c->kset), kb[c->rank], keys.p, kb.data()));
		CL_TRY(c->X.all_gather_v(c->X.user, cl_kmer_set_counts(c->kset), cb[c->rank], counts.p, cb.data()));
		cl_kmer_set_free(c->kset); c->kset = nullptr;
		CL_TRY(cl_kmer_set_create(ctx, keys.p, counts.p, n_all, c->P.k, &c->kset));
	}
	if (c->n_reads_total >= (1ull << 30)) return cl_fail(ctx, CL_E_UNSUPPORTED, "cl_compressor: >= 2^30 reads (reference ids are 30-bit, hm_compact.h:545-552)");
	st.n_reads = c->n_reads_total;
	c->gstats = st;
	// host scalars of compression.cpp:443,501-503 and the acceptor's decisions (one stream over the whole input, a6)
	const HostScalars hs = host_scalars(st, c->P, c->n_reads_total, c->genome_seqs, c->genome_len);
	c->mean_read_len = hs.mean_read_len; c->sparse_range = hs.sparse_range;
	c->h_accept.assign(c->n_reads_local, 1);
	CL_TRY(accept_stream(c->P, 0, c->n_reads_total, c->sparse_range, c->first_read, c->n_reads_local, c->h_accept.data()));
	c->phase = 1;
	if (stats) *stats = st;
	return CL_OK;
}

// ---- pass 2a --------------------------------------------------------------------------------------------------------
// Reference-genome mode (reference_genome.cpp:391-419, reads_sim_graph.cpp:295-322): the overlapping pieces of the genome are
// reference reads 0 .. n_pseudo-1 — always accepted, their k-mer lists not capped — ahead of the first read of the input.
extern "C" cl_status cl_compressor_pseudo_reads(cl_compressor* c, const cl_reads* pseudo)
{
	if (!c || !pseudo) return CL_E_INVALID;
	cl_ctx* ctx = c->ctx;
	if (c->phase != 1 || c->refs_chunk != 0 || c->n_pseudo) return cl_fail(ctx, CL_E_INVALID, "cl_compressor_pseudo_reads: once, after count_finish and before the first refs_add");
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	const uint32_t n = pseudo->n_reads;
	if (!n) return CL_OK;
	// Sharded reads: every rank is given the same pseudo reads; they are reference reads 0 .. n-1 of the replicated store, and rank 0
	// — whose references come first in the gather of pass 2a — is the one that contributes them and their index entries.  The
	// other ranks only note their number (reference ids, the coder's first read id and the acceptor's stream start behind them).
	if (c->world == 1 || c->rank == 0)
	{
		DevBuf<uint8_t> accept; DEV_ALLOC(ctx, accept, n);
		HIP_TRY(ctx, hipMemsetAsync(accept.p, 1, n, ctx->stream));
		HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
		Handle<cl_kmer_lists, cl_kmer_lists_free> lists;
		CL_TRY(cl_accepted_kmers(ctx, c->kset, pseudo, c->P.k, c->P.f, lists.out()));
		CL_TRY(append_index_entries(ctx, lists, accept.p, 0, c->pair_ids, c->pair_refs));
		cl_reads* piece = nullptr;
		CL_TRY(cl_reads_select(ctx, pseudo, accept.p, &piece));
		c->ref_pieces.push_back(piece);
		c->n_refs_local = n;
	}
	c->n_pseudo = n;
	// the acceptor's stream with the pseudo reads in front (ref_reads_accepter.h:41-58): decisions of the real reads follow them
	return accept_stream(c->P, n, c->n_reads_total, c->sparse_range, c->first_read, c->n_reads_local, c->h_accept.data());
}

extern "C" cl_status cl_compressor_refs_add(cl_compressor* c, const cl_reads* chunk)
{
	if (!c || !chunk) return CL_E_INVALID;
	cl_ctx* ctx = c->ctx;
	if (c->phase != 1) return cl_fail(ctx, CL_E_INVALID, "cl_compressor_refs_add: call after count_finish and before refs_finish");
	if (c->refs_chunk >= c->chunk_reads.size() || c->chunk_reads[c->refs_chunk] != chunk->n_reads)
		return cl_fail(ctx, CL_E_INVALID, "cl_compressor_refs_add: chunks must come in the order and sizes of pass 1");
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	const uint32_t n = chunk->n_reads;
	DevBuf<uint8_t> accept;
	CL_TRY(accept_flags(ctx, c->h_accept.data() + c->refs_reads_seen, chunk, accept));
	// the chunk's reference reads first (a tenth of its reads with the sparse acceptor), THEIR accepted k-mers only: rounds 2-5 listed the
	// k-mers of every read of the chunk here and kept those of the accepted ones — 50 scans of a gigabase in a pass that nothing overlaps
	c->bounds.emplace_back();
	DEV_ALLOC(ctx, c->bounds.back(), (uint64_t)n + 1);
	uint32_t n_acc = 0;
	CL_TRY(cl_ref_bounds(ctx, accept.p, n, c->n_refs_local, c->bounds.back().p, &n_acc));
	cl_reads* piece = nullptr;
	CL_TRY(cl_reads_select(ctx, chunk, accept.p, &piece));
	c->ref_pieces.push_back(piece);
	if (n_acc)
	{
		Handle<cl_kmer_lists, cl_kmer_lists_free> lists;
		CL_TRY(cl_accepted_kmers(ctx, c->kset, piece, c->P.k, c->P.f, lists.out()));
		DevBuf<uint8_t> all; DEV_ALLOC(ctx, all, n_acc);
		HIP_TRY(ctx, hipMemsetAsync(all.p, 1, n_acc, ctx->stream));            // (every read of the piece is a reference read: ref = base + its index)
		CL_TRY(append_index_entries(ctx, lists, all.p, c->n_refs_local, c->pair_ids, c->pair_refs));
	}
	c->n_refs_local += n_acc;
	c->refs_reads_seen += n; ++c->refs_chunk;
	return CL_OK;
}

// this rank's reference reads (arena pk / iv / ln: words, nr reads) and index entries all-gathered in rank order; reference ids become
// global.  On return the arena and c->pair_ids / c->pair_refs hold everybody's, nr and n_pairs their numbers.
static cl_status gather_refs(cl_compressor* c, DevBuf<uint64_t>& pk, DevBuf<uint32_t>& iv, DevBuf<uint32_t>& ln, uint64_t words, uint32_t& nr, uint64_t& n_pairs)
{
	cl_ctx* ctx = c->ctx; const uint32_t W = c->world;
	uint64_t mine[4] = { nr, words, c->pair_ids.n, 0 };
	std::vector<uint64_t> all((size_t)W * 4);
	CL_TRY(c->X.all_gather_host(c->X.user, mine, 4, all.data()));
	std::vector<uint64_t> b_pk(W), b_iv(W), b_ln(W), b_pr(W); uint64_t t_words = 0, t_reads = 0, t_pairs = 0;
	for (uint32_t r = 0; r < W; ++r)
	{
		const uint64_t* a = &all[(size_t)r * 4];
		if (r < c->rank) c->ref_base += (uint32_t)a[0];
		t_reads += a[0]; t_words += a[1]; t_pairs += a[2];
		b_ln[r] = a[0] * 4; b_pk[r] = a[1] * 8; b_iv[r] = a[1] * 4; b_pr[r] = a[2] * 4;
	}
	if (t_reads >= (1ull << 30)) return cl_fail(ctx, CL_E_UNSUPPORTED, "cl_compressor: >= 2^30 reference reads");
	c->n_refs_total = (uint32_t)t_reads;
	// global reference ids: this rank's references follow those of the lower ranks (file order)
	if (c->ref_base)
	{
		if (c->pair_refs.n) LAUNCH(ctx, k_add_u32, grid_for(c->pair_refs.n, 256), 256, c->pair_refs.buf.p, c->pair_refs.n, c->ref_base);
		for (size_t i = 0; i < c->bounds.size(); ++i) { const uint64_t m = (uint64_t)c->chunk_reads[i] + 1; LAUNCH(ctx, k_add_u32, grid_for(m, 256), 256, c->bounds[i].p, m, c->ref_base); }
		HIP_TRY(ctx, hipGetLastError());
		HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	}
	DevBuf<uint64_t> g_pk; DevBuf<uint32_t> g_iv, g_ln, g_id, g_rf;
	DEV_ALLOC(ctx, g_pk, t_words + 1); DEV_ALLOC(ctx, g_iv, t_words + 1); DEV_ALLOC(ctx, g_ln, t_reads + 1); DEV_ALLOC(ctx, g_id, t_pairs + 1); DEV_ALLOC(ctx, g_rf, t_pairs + 1);
	CL_TRY(c->X.all_gather_v(c->X.user, pk.p, b_pk[c->rank], g_pk.p, b_pk.data()));
	CL_TRY(c->X.all_gather_v(c->X.user, iv.p, b_iv[c->rank], g_iv.p, b_iv.data()));
	CL_TRY(c->X.all_gather_v(c->X.user, ln.p, b_ln[c->rank], g_ln.p, b_ln.data()));
	CL_TRY(c->X.all_gather_v(c->X.user, c->pair_ids.buf.p, b_pr[c->rank], g_id.p, b_pr.data()));
	CL_TRY(c->X.all_gather_v(c->X.user, c->pair_refs.buf.p, b_pr[c->rank], g_rf.p, b_pr.data()));
	pk = std::move(g_pk); iv = std::move(g_iv); ln = std::move(g_ln);
	c->pair_ids.buf = std::move(g_id); c->pair_refs.buf = std::move(g_rf); n_pairs = t_pairs;
	nr = (uint32_t)t_reads;
	return CL_OK;
}

extern "C" cl_status cl_compressor_refs_finish(cl_compressor* c)
{
	if (!c) return CL_E_INVALID;
	cl_ctx* ctx = c->ctx;
	if (c->phase != 1 || c->refs_chunk != c->chunk_reads.size()) return cl_fail(ctx, CL_E_INVALID, "cl_compressor_refs_finish: every chunk of pass 1 must have been listed");
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	// this rank's reference reads as one arena
	uint64_t words = 0; uint32_t nr = 0;
	for (auto* p : c->ref_pieces) { words += p->total_words; nr += p->n_reads; }
	DevBuf<uint64_t> pk; DevBuf<uint32_t> iv, ln; DEV_ALLOC(ctx, pk, words + 1); DEV_ALLOC(ctx, iv, words + 1); DEV_ALLOC(ctx, ln, (uint64_t)nr + 1);
	{
		uint64_t wo = 0; uint32_t ro = 0;
		for (auto* p : c->ref_pieces)
		{
			if (p->total_words) { HIP_TRY(ctx, hipMemcpyAsync(pk.p + wo, p->packed.p, p->total_words * 8, hipMemcpyDeviceToDevice, ctx->stream)); HIP_TRY(ctx, hipMemcpyAsync(iv.p + wo, p->inv.p, p->total_words * 4, hipMemcpyDeviceToDevice, ctx->stream)); }
			if (p->n_reads) HIP_TRY(ctx, hipMemcpyAsync(ln.p + ro, p->lens.p, (uint64_t)p->n_reads * 4, hipMemcpyDeviceToDevice, ctx->stream));
			wo += p->total_words; ro += p->n_reads;
		}
		HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
		for (auto* p : c->ref_pieces) cl_reads_free(p);
		c->ref_pieces.clear();
	}
	c->ref_base = 0; c->n_refs_total = nr;
	if (ctx->overlaps)
	{	// reference id -> read index, once, from the chunks' bounds (one rank, no pseudo reads: refused below otherwise)
		if (c->world > 1 || c->n_pseudo) return cl_fail(ctx, CL_E_UNSUPPORTED, "cl_ctx_set_overlaps: not with reads sharded over ranks or the pseudo reads of a reference genome (their reference ids are not reads of this input)");
		if (nr) { DEV_ALLOC(ctx, c->ref_read, nr); HIP_TRY(ctx, hipMemsetAsync(c->ref_read.p, 0xff, (uint64_t)nr * 4, cl_launch_stream(ctx))); }
		uint64_t g = 0;
		for (size_t i = 0; i < c->bounds.size(); ++i) { if (nr) CL_TRY(overlaps_ref_reads(ctx, c->bounds[i].p, c->chunk_reads[i], (uint32_t)g, c->ref_read.p, nr)); g += c->chunk_reads[i]; }
		HIP_TRY(ctx, hipStreamSynchronize(cl_launch_stream(ctx)));
	}
	if (ctx->mappings)
	{	// a record's target is a piece of the genome, lifted by the geometry: one rank, pseudo reads, and the geometry they were cut by
		if (c->world > 1) return cl_fail(ctx, CL_E_UNSUPPORTED, "cl_ctx_set_mappings: not with reads sharded over ranks (the records of the ranks are not merged yet)");
		if (!c->n_pseudo) return cl_fail(ctx, CL_E_INVALID, "cl_ctx_set_mappings: needs the pseudo reads of a reference genome (cl_compressor_pseudo_reads)");
		if (!c->has_map_geom) return cl_fail(ctx, CL_E_INVALID, "cl_ctx_set_mappings: needs the geometry of the pseudo reads (cl_compressor_genome_geometry)");
	}
	// the CIGARs are those of the mapping records: made in their hook, refused wherever they are
	if (ctx->cigars && !ctx->mappings) return cl_fail(ctx, CL_E_INVALID, "cl_ctx_set_cigars: needs the mapping records (cl_ctx_set_mappings)");
	if (ctx->cigars_coded && !ctx->cigars) return cl_fail(ctx, CL_E_INVALID, "cl_ctx_set_cigars_coded: needs the CIGARs (cl_ctx_set_cigars)");
	if (ctx->pileup)
	{	// a column lies on a piece of the genome, placed by the geometry: one rank, pseudo reads, and the geometry they were cut by
		if (c->world > 1) return cl_fail(ctx, CL_E_UNSUPPORTED, "cl_ctx_set_pileup: not with reads sharded over ranks (the tables of the ranks are not added yet)");
		if (!c->n_pseudo) return cl_fail(ctx, CL_E_INVALID, "cl_ctx_set_pileup: needs the pseudo reads of a reference genome (cl_compressor_pseudo_reads)");
		if (!c->has_map_geom) return cl_fail(ctx, CL_E_INVALID, "cl_ctx_set_pileup: needs the geometry of the pseudo reads (cl_compressor_genome_geometry)");
	}
	uint64_t n_pairs = c->pair_ids.n;
	if (c->world > 1) CL_TRY(gather_refs(c, pk, iv, ln, words, nr, n_pairs));
	CL_TRY(cl_reads_from_arena(ctx, pk.p, iv.p, ln.p, nr, &c->refs));
	pk.release(); iv.release(); ln.release();
	if (ctx->pileup) CL_TRY(pileup_for_compressor(c));                        // the ONE table: the pieces are reads 0 .. n_pseudo-1 of the arena just made
	CL_TRY(cl_index_build_pairs(ctx, c->kset, c->pair_ids.buf.p, c->pair_refs.buf.p, n_pairs, nullptr, 0, c->n_refs_total, c->n_pseudo, c->P.cs, &c->index));
	c->pair_ids.buf.release(); c->pair_refs.buf.release(); c->pair_ids.n = c->pair_refs.n = 0;
	// the coders of this rank's model domain; cur_read_id starts at the global index of the first read, so that the ids of
	// references from lower ranks fit the byte count the coder derives from it (dna_coder.cpp:26-63)
	CL_TRY(cl_dna_coder_create(ctx, c->P.c, c->P.level, (uint32_t)c->first_read + c->n_pseudo, &c->dna));     // (pseudo reads count as reads 0 .. n_pseudo-1, dna_coder.cpp:1242-1250)
	if (c->has_qual)
	{
		cl_ctx* qc = (c->P.level <= 1) ? c->qctx : ctx;        // levels 2 and 3 need the edit scripts: same stream as the DNA path
		const cl_status s = cl_qual_coder_create(qc, &c->Q, &c->qual);
		if (s != CL_OK) return cl_fail(ctx, s, std::string("quality coder: ") + cl_last_error(qc));
		CL_TRY(cl_qual_coder_set_domain_symbols(c->qual, c->qual_domain_symbols));
	}
	c->phase = 2;
	return CL_OK;
}

// ---- pass 2b --------------------------------------------------------------------------------------------------------
cl_status compressor_tuple_streams(cl_compressor* c, cl_ctx* ctx, size_t idx, const cl_reads* reads, const uint32_t* h_pack_bounds, uint32_t n_packs, TupleStreams& out)
{
	Handle<cl_kmer_lists, cl_kmer_lists_free> lists;            // a4: accepted k-mers per read
	CL_TRY(cl_accepted_kmers(ctx, c->kset, reads, c->P.k, c->P.f, lists.out()));
	uint64_t g = c->first_read; for (size_t i = 0; i < idx; ++i) g += c->chunk_reads[i];      // the chunk's first read in the whole input
	return tuple_streams(ctx, &c->P, lists, c->index, c->refs, reads, c->bounds[idx].p, h_pack_bounds, n_packs, g, c->ref_read.p, c->ref_read.p ? c->n_refs_total : 0u, c->has_map_geom ? &c->map_geom : nullptr, c->pileup, out);
}

extern "C" cl_status cl_compressor_encode(cl_compressor* c, const cl_reads* reads, const uint8_t* d_quals, const uint64_t* d_base_off,
                                          const uint32_t* h_part_bounds, uint32_t n_parts, const uint32_t* h_pack_bounds, uint32_t n_packs,
                                          uint8_t* d_dna_out, uint64_t dna_cap, uint64_t* h_dna_part_sizes,
                                          uint8_t* d_qual_out, uint64_t qual_cap, uint64_t* h_qual_part_sizes, cl_compress_info* info)
{
	if (!c || !reads || !h_part_bounds || !h_pack_bounds || !info) return CL_E_INVALID;
	cl_ctx* ctx = c->ctx;
	if (c->phase != 2) return cl_fail(ctx, CL_E_INVALID, "cl_compressor_encode: call after refs_finish");
	if (c->enc_chunk >= c->chunk_reads.size() || c->chunk_reads[c->enc_chunk] != reads->n_reads)
		return cl_fail(ctx, CL_E_INVALID, "cl_compressor_encode: chunks must come in the order and sizes of pass 1");
	if (c->has_qual && (!d_quals || !d_base_off || !h_qual_part_sizes || !d_qual_out)) return cl_fail(ctx, CL_E_INVALID, "cl_compressor_encode: quality stream without qualities");
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	memset(info, 0, sizeof(*info));
	const uint32_t n = reads->n_reads;
	const size_t idx = c->enc_chunk;
	info->n_reads = n; info->n_bases = reads->total_bases; info->tot_kmers = c->gstats.tot_kmers; info->n_kept_kmers = c->gstats.n_unique_counted;
	info->n_refs = c->n_refs_total; info->sparse_range = c->sparse_range;
	std::unique_ptr<Prepared> job;                         // stage A result: announced (taken from the look-ahead) or made here
	CL_TRY(lookahead_take(c, reads, job));
	// the chunk leaves the look-ahead window whatever happens below (lanes may go on to the next announced chunk)
	struct Advance { cl_compressor* c; size_t idx; ~Advance() { { std::lock_guard<std::mutex> l(c->la.lane_mu); c->la.prepared.erase(idx); c->bounds[idx].release(); c->enc_chunk = idx + 1; } c->la.lane_cv.notify_all(); } } adv{ c, idx };
	if (!n) return CL_OK;
	if (ctx->digest)
	{	// the content digest of the chunk, from the input, at its reads' indices in the whole input, before the coders start
		uint64_t g = c->first_read; for (size_t i = 0; i < idx; ++i) g += c->chunk_reads[i];
		CL_TRY(digest_chunk(ctx, reads, c->has_qual ? &c->Q : nullptr, d_quals, d_base_off, g));
	}
	if (ctx->digest_values && c->has_qual)
	{	// the qual-values digest of the chunk, next to them
		uint64_t g = c->first_read; for (size_t i = 0; i < idx; ++i) g += c->chunk_reads[i];
		CL_TRY(digest_values_chunk(ctx, reads, &c->Q, d_quals, d_base_off, g));
	}
	if (ctx->report) CL_TRY(report_chunk(ctx, reads, c->has_qual ? &c->Q : nullptr, d_quals, d_base_off));   // the content report of the chunk, from the same input
	struct HooksOff { cl_compressor* c; ~HooksOff() { cl_dna_set_before_tail(c->dna, nullptr); cl_qual_set_before_tail(c->qual, nullptr); } } hooks_off{ c };
	ChunkCoder coder(ctx, c->P.level, c->dna, c->qual, ChunkIO{ reads, d_quals, d_base_off, h_part_bounds, n_parts, d_dna_out, dna_cap, h_dna_part_sizes, d_qual_out, qual_cap, h_qual_part_sizes, info });
	lookahead_quality(c, job.get(), coder);
	coder.start_quality();
	CL_TRY(lookahead_dna(c, job.get()));
	if (!job)
	{
		job = std::make_unique<Prepared>();
		CL_TRY(compressor_tuple_streams(c, ctx, idx, reads, h_pack_bounds, n_packs, *job));
	}
	info->n_anchors = job->n_anchors; info->tuple_bytes = job->es_bytes;
	return coder.code(c->refs, *job);
}

// model domains of the quality stream (cl_qual_coder_set_domain_symbols): before anything of pass 2b has seen the coder
extern "C" cl_status cl_compressor_set_qual_domain_symbols(cl_compressor* c, uint64_t n)
{
	if (!c) return CL_E_INVALID;
	if (!c->has_qual) return cl_fail(c->ctx, CL_E_INVALID, "cl_compressor_set_qual_domain_symbols: no quality stream");
	{
		std::lock_guard<std::mutex> l(c->la.lane_mu);
		if (c->enc_chunk || c->la.n_announced) return cl_fail(c->ctx, CL_E_INVALID, "cl_compressor_set_qual_domain_symbols: call before the first cl_compressor_encode / cl_compressor_prepare_parts");
	}
	c->qual_domain_symbols = n;
	if (c->qual) { const cl_status s = cl_qual_coder_set_domain_symbols(c->qual, n); if (s != CL_OK) return cl_fail(c->ctx, s, std::string("quality coder: ") + cl_last_error(cl_qual_coder_ctx(c->qual))); }
	return CL_OK;
}
extern "C" cl_status cl_compressor_qual_domains(const cl_compressor* c, uint64_t* h_first_part, uint64_t cap, uint64_t* n_out)
{
	if (!c || !n_out) return CL_E_INVALID;
	if (!c->qual) return cl_fail(c->ctx, CL_E_INVALID, "cl_compressor_qual_domains: no quality coder (yet)");
	const cl_status s = cl_qual_coder_domains(c->qual, h_first_part, cap, n_out);
	return s == CL_OK ? CL_OK : cl_fail(c->ctx, s, "cl_compressor_qual_domains: capacity");
}

extern "C" cl_status cl_compressor_verified(const cl_compressor* c, uint64_t* reads, uint64_t* bases)
{
	return c ? cl_ctx_verified(c->ctx, reads, bases) : CL_E_INVALID;
}

extern "C" cl_status cl_compressor_digest(const cl_compressor* c, cl_digest* dna, cl_digest* qual)
{
	return c ? cl_ctx_digest(c->ctx, dna, qual) : CL_E_INVALID;
}
extern "C" cl_status cl_compressor_digest_values(const cl_compressor* c, cl_digest* out)
{
	return c ? cl_ctx_digest_values(c->ctx, out) : CL_E_INVALID;
}
extern "C" cl_status cl_compressor_report(const cl_compressor* c, cl_report* out)
{
	return c ? cl_ctx_report(c->ctx, out) : CL_E_INVALID;
}

// every context that codes for the compressor: its own (the DNA stream; the quality stream of levels 2 and 3) and the quality coder's
extern "C" cl_status cl_compressor_edit_profile(const cl_compressor* c, cl_edits* out)
{
	return c ? cl_ctx_edit_profile(c->ctx, out) : CL_E_INVALID;
}
extern "C" cl_status cl_compressor_overlaps(const cl_compressor* c, cl_overlap* h_out, uint64_t cap, uint64_t* n_out)
{
	return c ? cl_ctx_overlaps(c->ctx, h_out, cap, n_out) : CL_E_INVALID;
}
extern "C" cl_status cl_compressor_kmer_spectrum(const cl_compressor* c, cl_kspec* out)
{
	return c ? cl_ctx_kmer_spectrum(c->ctx, out) : CL_E_INVALID;
}
extern "C" cl_status cl_compressor_kmer_sketch(const cl_compressor* c, cl_sketch* out)
{
	return c ? cl_ctx_kmer_sketch(c->ctx, out) : CL_E_INVALID;
}
extern "C" cl_status cl_compressor_verified_streams(const cl_compressor* c, uint64_t* parts, uint64_t* symbols, uint64_t* bytes)
{
	if (!c) return CL_E_INVALID;
	uint64_t v[3] = { 0, 0, 0 };
	CL_TRY(cl_ctx_verified_streams(c->ctx, &v[0], &v[1], &v[2]));
	const cl_ctx* qc = c->qual ? cl_qual_coder_ctx(c->qual) : nullptr;
	if (qc && qc != c->ctx)
	{
		uint64_t q[3] = { 0, 0, 0 };
		CL_TRY(cl_ctx_verified_streams(qc, &q[0], &q[1], &q[2]));
		for (int i = 0; i < 3; ++i) v[i] += q[i];
	}
	if (parts) *parts = v[0];
	if (symbols) *symbols = v[1];
	if (bytes) *bytes = v[2];
	return CL_OK;
}

extern "C" cl_status cl_compressor_info(const cl_compressor* c, cl_kmer_stats* stats, uint64_t* first_read, uint64_t* n_reads_total, uint64_t* mean_read_len,
                                        uint32_t* sparse_range, uint32_t* n_refs_total)
{
	if (!c || c->phase < 1) return CL_E_INVALID;
	if (stats) *stats = c->gstats;
	if (first_read) *first_read = c->first_read;
	if (n_reads_total) *n_reads_total = c->n_reads_total;
	if (mean_read_len) *mean_read_len = c->mean_read_len;
	if (sparse_range) *sparse_range = c->sparse_range;
	if (n_refs_total) *n_refs_total = c->n_refs_total;
	return CL_OK;
}
