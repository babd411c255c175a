// objects.hpp — device-resident objects behind the opaque C-ABI handles.
#pragma once
#include "common.hpp"
#include <memory>

struct cl_reads {
	cl_ctx* ctx = nullptr;
	uint32_t n_reads = 0;
	uint64_t total_bases = 0, total_words = 0;
	DevBuf<uint64_t> packed;      // total_words + 1 (tail word), 32 bases per word, first base in bits 63..62
	DevBuf<uint32_t> inv;         // total_words + 1, bit 31-j = base j invalid (N or pad)
	DevBuf<uint64_t> word_off;    // n_reads + 1
	DevBuf<uint32_t> lens;        // n_reads
	DevBuf<uint8_t> has_n;        // n_reads
};

struct cl_kmer_set {
	cl_ctx* ctx = nullptr;
	uint32_t k = 0;
	uint64_t n = 0;
	DevBuf<uint64_t> keys;        // ascending
	DevBuf<uint32_t> counts;      // min(count, cs)
	DevBuf<uint64_t> slots;       // buckets of 4 x {key, rank}: 8 uint64 per bucket
	uint64_t bmask = 0;
};

struct cl_kmer_lists {
	cl_ctx* ctx = nullptr;
	uint32_t n_reads = 0;
	uint64_t total = 0;
	DevBuf<uint64_t> off;         // n_reads + 1
	DevBuf<uint64_t> kmers;       // k-mer values
	DevBuf<uint32_t> ids;         // rank in the set
	DevBuf<uint32_t> pos;         // start position in the read
	DevBuf<uint32_t> read;        // owning read of each entry
};

struct cl_index {
	cl_ctx* ctx = nullptr;
	uint32_t n_reads = 0, n_refs = 0, n_pseudo = 0;
	uint64_t n_keys = 0, n_entries = 0;
	DevBuf<uint32_t> ref_rank;    // n_reads + 1: number of reference reads before read i
	DevBuf<uint64_t> off;         // n_keys + 1 (CSR over set ranks)
	DevBuf<uint32_t> refs;        // reference ids, ascending inside a list
};

// key-range partitioning of k-mers (kmer.hip): histogram over the 4096 bins of the top 12 key bits, gather of a bin range
uint32_t cl_part_shift(uint32_t k);
cl_status cl_key_histogram(cl_ctx* ctx, const uint64_t* d_kmers, uint64_t n, uint32_t k, std::vector<uint64_t>& h_bins);
cl_status cl_key_gather(cl_ctx* ctx, const uint64_t* d_kmers, uint64_t n, uint32_t k, uint32_t b0, uint32_t b1, uint64_t* d_out, uint64_t expect);

// graph.hip: reference reads before each read of a chunk (the first half of cl_index_entries_of on its own)
cl_status cl_ref_bounds(cl_ctx* ctx, const uint8_t* d_accept, uint32_t n, uint32_t ref_base, uint32_t* d_bounds, uint32_t* n_accepted);

// expand.hip: cl_es_verify with the first differing base of the first bad read (~0u: its length or tuple count differs); es_bytes: the
// tuple bytes, for the achieved bytes/s of timed runs (0: not known)
cl_status cl_es_verify_at(cl_ctx* ctx, const cl_reads* reads, const cl_reads* refs, const uint8_t* d_es, const uint64_t* d_es_off, const uint32_t* d_es_ntuples,
                          uint64_t es_bytes, uint64_t* n_bad, uint32_t* first_bad, uint32_t* first_diff);

// digest.hip (cl_ctx_set_digest): the dna digest of a chunk whose first read is read `first_read` of the input and, with qparams, its qual
// digest, added to the context's totals; on the context's stream, from the input arena and quality bytes alone
cl_status digest_chunk(cl_ctx* ctx, const cl_reads* reads, const cl_qual_params* qparams, const uint8_t* d_quals, const uint64_t* d_base_off, uint64_t first_read);
// (cl_ctx_set_digest_values): the qual-values digest of the same chunk, from the input quality bytes alone (nothing with qparams null or mode none)
cl_status digest_values_chunk(cl_ctx* ctx, const cl_reads* reads, const cl_qual_params* qparams, const uint8_t* d_quals, const uint64_t* d_base_off, uint64_t first_read);
// report.hip (cl_ctx_set_report): the content report of the same chunk — the arena and, with qparams, the input quality bytes — added to the context's total
cl_status report_chunk(cl_ctx* ctx, const cl_reads* reads, const cl_qual_params* qparams, const uint8_t* d_quals, const uint64_t* d_base_off);
// edits.hip (cl_ctx_set_edit_profile): the edit-operation profile of a batch of tuple streams, added to the total of the context that made them
cl_status edit_profile_chunk(cl_ctx* ctx, const cl_reads* refs, const uint8_t* d_es, const uint64_t* d_es_off, uint32_t n_reads);
// kspec.hip (cl_ctx_set_kmer_spectrum): the count spectrum of one counted key range — the run starts of its n sorted keys — added to the context's total
cl_status kmer_spectrum_range(cl_ctx* ctx, const uint32_t* d_head_pos, uint64_t n_heads, uint64_t n);
// sketch.hip (cl_ctx_set_kmer_sketch): the MinHash sketch of one counted key range — its n sorted keys and the starts of their runs — merged into the context's
cl_status kmer_sketch_range(cl_ctx* ctx, const uint64_t* d_keys, const uint32_t* d_head_pos, uint64_t n_heads, uint64_t n);
// overlaps.hip (cl_ctx_set_overlaps): the overlap records of a batch of tuple streams whose first read is read `first_read` of the input, kept on the
// host by the context that made them; d_ref_read (n_ref_read entries, or null): reference id -> input index
cl_status overlaps_chunk(cl_ctx* ctx, const cl_reads* refs, const uint8_t* d_es, const uint64_t* d_es_off, uint32_t n_reads, uint64_t first_read, const uint32_t* d_ref_read, uint32_t n_ref_read);
// ... and that table's entries of one chunk: read i (input index first_read + i) is reference d_bounds[i] iff d_bounds[i + 1] > d_bounds[i] (n + 1 bounds)
cl_status overlaps_ref_reads(cl_ctx* ctx, const uint32_t* d_bounds, uint32_t n, uint32_t first_read, uint32_t* d_ref_read, uint32_t n_ref_read);
// ... and the records alone, ids untranslated, in a buffer made by the call (mappings.hip lifts them); rec_off (or null) takes the records'
// offsets per read, n_reads + 1 entries; overlaps_offsets: those offsets alone (the count and the prefix sum, no fill; n_reads > 0)
cl_status overlaps_records(cl_ctx* ctx, const cl_reads* refs, const uint8_t* d_es, const uint64_t* d_es_off, uint32_t n_reads, uint64_t first_read, DevBuf<cl_overlap>& out, uint64_t* n_out,
                           DevBuf<uint64_t>* rec_off = nullptr);
cl_status overlaps_offsets(cl_ctx* ctx, const char* who, const cl_reads* refs, const uint8_t* d_es, const uint64_t* d_es_off, uint32_t n_reads, uint32_t max_blocks, DevBuf<uint64_t>& rec_off,
                           uint64_t* n_out);
// cigars.hip (cl_ctx_set_cigars, from mappings_chunk): the CIGARs of a batch's records on reference ids below id_limit — the genome's pieces,
// the records the lift keeps, in their order — copied to the host and kept by the context that made them; d_rec_off / n_rec: that batch's
// record offsets per read and record count (overlaps_records); n_lifted: the records the lift kept
cl_status cigars_chunk(cl_ctx* ctx, const cl_reads* refs, const uint8_t* d_es, const uint64_t* d_es_off, uint32_t n_reads, uint64_t first_read, uint32_t id_limit, const uint64_t* d_rec_off,
                       uint64_t n_rec, uint64_t n_lifted);
// cigar_coder.hip (cl_cigars_pack, and cigars_chunk under cl_ctx_set_cigars_coded): the segments (cigar_coder.hpp) of n_ops words in device memory appended
// to out; a knob of 0 is its default; out is unchanged when the call fails
cl_status cigars_pack_device(cl_ctx* ctx, const char* who, const uint32_t* d_ops, uint64_t n_ops, uint32_t part_ops, uint32_t seg_ops, std::vector<uint8_t>& out, uint64_t* n_segments, uint64_t* n_escapes);
// mappings.hip (cl_ctx_set_mappings): the records of a batch whose target is a piece of the reference genome, lifted to the genome's sequences
// (geom: mappings.hpp, tables on the device; null is an error) and kept on the host by the context that made them
struct MapGeom;
cl_status mappings_chunk(cl_ctx* ctx, const cl_reads* refs, const uint8_t* d_es, const uint64_t* d_es_off, uint32_t n_reads, uint64_t first_read, const MapGeom* geom);
// pileup.hip (cl_ctx_set_pileup): a batch of tuple streams added to the compressor's table `p` (null is an error) by a launch on `ctx`, the context that
// made them; and that table made for a compressor whose references are finished, from the geometry kept for the mappings
struct cl_compressor;
cl_status pileup_chunk(cl_ctx* ctx, cl_pileup* p, const cl_reads* refs, const uint8_t* d_es, const uint64_t* d_es_off, uint32_t n_reads);
cl_status pileup_for_compressor(cl_compressor* c);
const cl_qual_params* cl_qual_coder_params(const cl_qual_coder* q);     // qual.hip: the parameters the coder was created with

// the DNA coder's state-independent half ahead of time (dna.hip): lookahead.hip walks the NEXT chunk's tuples from the hook that
// cl_dna_encode calls before it waits for its last interval coding
#include <functional>
struct cl_dna_coder;
cl_status cl_dna_walk_ahead(cl_ctx* ctx, cl_dna_coder* D, const cl_reads* refs, const uint8_t* d_es, const uint64_t* d_es_off, const uint32_t* d_es_ntuples, uint32_t n_reads);
void cl_dna_set_before_tail(cl_dna_coder* D, std::function<cl_status()> fn);
// the model-independent half of a batch (walks; with part bounds also layout, sort and context runs) on any context — see dna.hip
struct DnaWalked;
cl_status cl_dna_prepare_batch(cl_ctx* ctx, cl_dna_coder* D, const cl_reads* refs, const uint8_t* d_es, const uint64_t* d_es_off, const uint32_t* d_es_ntuples, uint32_t n_reads,
                               uint32_t prev_types, uint32_t read_id, const uint32_t* h_part_bounds, uint32_t n_parts, DnaWalked** out, uint32_t* prev_types_out);
void cl_dna_walked_free(DnaWalked* W);
void cl_dna_set_ahead(cl_dna_coder* D, DnaWalked* W);               // takes W: the next cl_dna_encode uses it if it is the batch it was made for
void cl_dna_coder_state(const cl_dna_coder* D, uint32_t* prev_types, uint32_t* read_id);
cl_status cl_dna_model_read(const cl_dna_coder* D, uint32_t family, uint64_t context, uint32_t* out);   // behind cl_dna_coder_model (capi.hip)
cl_status cl_qual_model_read(const cl_qual_coder* Q, uint32_t family, uint64_t context, uint32_t* out, uint32_t cap, uint32_t* n_out);   // behind cl_qual_coder_model (capi.hip)
// the read-type history a batch hands to the next one (types of its last four reads after `prev_types`): from the first tuple of those reads alone
cl_status cl_dna_batch_types(cl_ctx* ctx, const uint8_t* d_es, const uint64_t* d_es_off, uint32_t n_reads, uint64_t es_bytes, uint32_t prev_types, uint32_t* out);
// the same for the quality coder (qual.hip): symbols, sort by context, context runs of a batch, on any context
struct QualPrepared;
cl_status cl_qual_prepare_batch(cl_ctx* ctx, cl_qual_coder* Q, const cl_reads* R, const uint8_t* d_quals, const uint64_t* d_qual_off,
                                const uint8_t* d_flags, const uint32_t* h_part_bounds, uint32_t n_parts, QualPrepared** out);
void cl_qual_prepared_free(QualPrepared* P);
void cl_qual_set_ahead(cl_qual_coder* Q, QualPrepared* P);
// the model half of the NEXT batch (takes W / P) while the interval coders of the current one run: from the coders' before_tail hooks
cl_status cl_dna_evolve_ahead(cl_ctx* ctx, cl_dna_coder* D, const cl_reads* refs, const uint8_t* d_es, const uint64_t* d_es_off, const uint32_t* d_es_ntuples, uint32_t n_reads,
                              const uint32_t* h_part_bounds, uint32_t n_parts, DnaWalked* W);
cl_status cl_qual_evolve_ahead(cl_ctx* ctx, cl_qual_coder* Q, const cl_reads* R, const uint8_t* d_quals, const uint64_t* d_qual_off, const uint32_t* h_part_bounds, uint32_t n_parts, QualPrepared* P);
void cl_qual_set_before_tail(cl_qual_coder* Q, std::function<cl_status()> fn);
constexpr cl_status CL_HOOK_RETRY = (cl_status)1000;     // a before_tail hook: "nothing to do yet" — asked again while the batch's interval coders run
