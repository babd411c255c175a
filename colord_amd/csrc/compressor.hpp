// compressor.hpp — cl_compressor: the state of a chunked compression between calls.  stream.hip takes it through the passes (and the
// exchanges of sharded reads); lookahead.hip is the pipeline that works on announced chunks ahead of the calls that code them.
#pragma once
#include "pass_steps.hpp"
#include "mappings.hpp"

// An announced chunk on its way through the look-ahead: stage A by an encode lane, then the coders' model-independent halves.
struct Prepared : TupleStreams {
	const cl_reads* reads = nullptr; std::vector<uint32_t> packs;
	cl_status status = CL_OK; std::string err;
	std::map<std::string, KernelTime> times;      // kernel times of the lane for this chunk (merged into the caller's context)
	bool done = false;
	// the model-independent half of the DNA coder for this chunk (tuple walks, and with part bounds the sort by context), made by
	// the compressor's preparation thread beside the coding of the chunk before (cl_dna_prepare_batch)
	std::vector<uint32_t> parts; DnaWalked* walked = nullptr; bool dna_done = false; std::map<std::string, KernelTime> dna_times;
	// ... and of the quality coder (symbols, sort by context), which needs the input only (level 1: no flags from the edit scripts)
	const uint8_t* d_quals = nullptr; const uint64_t* d_base_off = nullptr; QualPrepared* qprep = nullptr; bool q_done = false; std::map<std::string, KernelTime> q_times;
	~Prepared() { if (walked) cl_dna_walked_free(walked); if (qprep) cl_qual_prepared_free(qprep); }
};

// wall-clock laps: each call adds the time since the last one (or since construction) to `acc`
struct Lap {
	static std::chrono::steady_clock::time_point now() { return std::chrono::steady_clock::now(); }
	std::chrono::steady_clock::time_point t = now();
	void operator()(double& acc) { const auto n = now(); acc += std::chrono::duration<double>(n - t).count(); t = n; }
};

// Look-ahead (cl_compressor_prepare): stage A of announced chunks — candidates, anchors, alignments, tuple streams, none of which
// depends on an earlier chunk's coders — runs on the compressor's own contexts ("encode lanes", one worker thread each) while the
// caller's thread codes the chunks before them; preparation workers then make the coders' model-independent halves.  Everything
// below is guarded by lane_mu unless it says otherwise.
struct LookAhead {
	std::mutex lane_mu; std::condition_variable lane_cv;
	std::deque<size_t> lane_queue;                   // announced chunk indices not yet started, ascending
	std::map<size_t, std::unique_ptr<Prepared>> prepared;
	std::vector<std::thread> lane_threads; std::vector<cl_ctx*> lane_ctx;
	size_t n_announced = 0; bool lane_stop = false;
	// DNA preparation: workers (contexts of their own) that CLAIM the chunks in order; the two scalars that chain from chunk to chunk — the
	// types of the last four reads, the read count — are advanced at the claim (cl_dna_batch_types: a few bytes of the tuple streams), so
	// the chunks themselves are prepared side by side
	std::vector<std::thread> prep_threads; std::vector<cl_ctx*> prep_ctxs; std::mutex prep_claim_mu;
	size_t prep_next = 0; bool prep_on = false, prep_broken = false; uint32_t prep_types = 0, prep_read_id = 0;
	std::thread qprep_thread; size_t qprep_next = 0; bool qprep_on = false;
	// chunks whose model half is done ahead of their encode call (first not yet done; the thread that codes only), and how far ahead that
	// may go: with the reference's parts the interval coders of a chunk take 1.3 s, those of `evolve_depth` + 1 chunks run side by side
	size_t dna_evolved_upto = 0, qual_evolved_upto = 0; uint32_t evolve_depth = 0;
	bool no_evolve_ahead = false;                    // COLORD_HIP_NO_EVOLVE_AHEAD, read with the other switches when the look-ahead is set up
	uint32_t n_dna_ahead = 0, n_qual_ahead = 0, n_dna_prep = 0, n_qual_prep = 0;      // (statistics: COLORD_HIP_STREAM_DEBUG)
	double w_lane_idle = 0, w_lane_work = 0, w_enc_lane = 0, w_enc_prep = 0, w_enc_qprep = 0, w_prep_idle = 0, w_prep_work = 0;   // seconds: who waited for whom
	void stop();                                     // ends and joins the workers; what they prepared goes back to the pool
	void report(size_t n_chunks) const;              // the two [stream] lines of COLORD_HIP_STREAM_DEBUG
};

struct cl_compressor {
	cl_ctx* ctx = nullptr; cl_ctx* qctx = nullptr;
	cl_compress_params P{}; bool has_qual = false; cl_qual_params Q{};
	cl_exchange X{}; uint32_t rank = 0, world = 1;
	int phase = 0;                                  // 0 counting, 1 counted, 2 references listed, 3 encoding
	// pass 1
	Grow<uint64_t> kmers; uint64_t expected_bases = 0;
	std::vector<uint32_t> chunk_reads; uint64_t n_reads_local = 0, n_bases_local = 0;
	cl_kmer_set* kset = nullptr; cl_kmer_stats gstats{};
	uint64_t n_reads_total = 0, first_read = 0, mean_read_len = 0; uint32_t sparse_range = 0;
	uint64_t genome_seqs = 0, genome_len = 0; uint32_t n_pseudo = 0;      // reference-genome mode (compression.cpp:405-447)
	std::vector<uint8_t> h_accept;                  // acceptor decisions of this rank's reads
	// pass 2a
	size_t refs_chunk = 0; uint64_t refs_reads_seen = 0; uint32_t n_refs_local = 0;
	std::vector<cl_reads*> ref_pieces;
	Grow<uint32_t> pair_ids, pair_refs;
	std::vector<DevBuf<uint32_t>> bounds;           // per chunk: n_reads + 1, reference reads before each read
	cl_reads* refs = nullptr; cl_index* index = nullptr; uint32_t ref_base = 0, n_refs_total = 0;
	DevBuf<uint32_t> ref_read;                      // cl_ctx_set_overlaps: reference id -> index of that read in the input (n_refs_total entries), made in refs_finish
	DevBuf<uint64_t> map_seq_len; DevBuf<uint32_t> map_piece_first; // cl_compressor_genome_geometry: the tables of the pseudo reads' geometry (mappings.hpp) ...
	MapGeom map_geom{}; bool has_map_geom = false;  // ... and the geometry over them, for the lifts of cl_ctx_set_mappings
	std::vector<uint64_t> map_seq_len_h;            // ... and the sequence lengths on the host, for the table of cl_ctx_set_pileup
	cl_pileup* pileup = nullptr;                    // cl_ctx_set_pileup: the ONE table of this compressor, made in refs_finish; every lane adds into it (pileup.hip)
	cl_dna_coder* dna = nullptr; cl_qual_coder* qual = nullptr;
	uint64_t qual_domain_symbols = 0;               // cl_compressor_set_qual_domain_symbols: handed to the quality coder when it is created
	// pass 2b
	size_t enc_chunk = 0;                           // (written under la.lane_mu: the look-ahead's windows move with it)
	LookAhead la;
	~cl_compressor();
};

// stage A of chunk `idx` on `ctx` (stream.hip)
cl_status compressor_tuple_streams(cl_compressor* c, cl_ctx* ctx, size_t idx, const cl_reads* reads, const uint32_t* h_pack_bounds, uint32_t n_packs, TupleStreams& out);
// lookahead.hip, for cl_compressor_encode — the chunk at c->enc_chunk, in this order:
// the announced job once its lane and the preparation workers are through with it (null: the chunk was not announced)
cl_status lookahead_take(cl_compressor* c, const cl_reads* reads, std::unique_ptr<Prepared>& job);
// before the quality thread starts: the job's prepared half goes to the quality coder, whose hook evolves the chunks ahead
void lookahead_quality(cl_compressor* c, Prepared* job, const ChunkCoder& coder);
// before cl_dna_encode: what the lane and the DNA preparation made of the job (if any) is adopted; the DNA coder's hook
cl_status lookahead_dna(cl_compressor* c, Prepared* job);
