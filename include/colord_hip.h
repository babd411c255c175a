/* colord_hip.h — C ABI of the MI355X-native CoLoRd hot path (libcolord_hip.so).
 *
 * The reference (refresh-bio/colord v1.2.1) has no FFI layer: its seams are the C++ stage objects that
 * `runCompression` (src/colord/compression.cpp:344-785) wires together.  Every entry point below names
 * the reference seam it replaces so that a host driver shaped like `runCompression` can call them 1:1.
 * See INTEGRATION.md for the binding a reference maintainer would add.
 *
 * Conventions
 *  - plain C, no C++/torch types; every function returns cl_status (0 = ok, <0 = error, text via
 *    cl_last_error); nothing throws, nothing calls exit().
 *  - pointers named d_* are DEVICE pointers (hipMalloc / torch CUDA tensor data_ptr), h_* are host.
 *  - one cl_ctx per GPU; calls on different contexts are thread-safe, calls on one context are
 *    serialised by the caller.  All kernels of a context run on the context's own HIP stream; a call
 *    returns after its results are complete (it synchronises that stream).
 *  - objects (cl_reads, cl_kmer_set, ...) are owned by the context and freed by their *_free or by
 *    cl_ctx_destroy.
 *  - bases are 2-bit codes A=0 C=1 G=2 T=3 (N=4 in the 1-byte input form), k-mers are uint64 with the
 *    first base in the most significant used bits (src/colord/in_reads.h:30-74), k <= 28
 *    (src/colord/arg_parse.cpp:471).
 */
#ifndef COLORD_HIP_H
#define COLORD_HIP_H
#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef int32_t cl_status;
enum {
	CL_OK = 0,
	CL_E_INVALID = -1,      /* bad argument */
	CL_E_HIP = -2,          /* HIP runtime error (text in cl_last_error) */
	CL_E_CAPACITY = -3,     /* caller buffer too small; the needed element count was returned */
	CL_E_NOMEM = -4,
	CL_E_UNSUPPORTED = -5,
	CL_E_MISMATCH = -6      /* cl_ctx_set_verify: a read is not rebuilt from its edit script (text names the read and the base);
	                         * cl_ctx_set_verify_streams: a coded part does not decode to its models' intervals or does not end at its
	                         * size (text names the stream, the part, its symbols and bytes, and the first such symbol or the byte counts) */
};

typedef struct cl_ctx cl_ctx;
typedef struct cl_reads cl_reads;         /* packed read arena on device */
typedef struct cl_kmer_set cl_kmer_set;   /* filtered k-mer set (CKmerFilter) */
typedef struct cl_kmer_lists cl_kmer_lists; /* per-read accepted k-mers (getAcceptedKmers) */
typedef struct cl_index cl_index;         /* k-mer -> reference reads (CKmersToReads) */

/* ---- context ---------------------------------------------------------------------------------- */
cl_status cl_ctx_create(int device, cl_ctx** out);
void cl_ctx_destroy(cl_ctx* ctx);
const char* cl_last_error(const cl_ctx* ctx);
/* HIP stream the context launches on (hipStream_t as void*), for callers that time with HIP events. */
void* cl_ctx_stream(cl_ctx* ctx);
/* Wall-clock free device timing of the LAST call's dominant kernel, measured with HIP events on the
 * context stream: *ms = elapsed milliseconds, *launches = number of launches it covers. */
cl_status cl_ctx_last_kernel_ms(const cl_ctx* ctx, const char* kernel, double* ms, uint32_t* launches);
/* Kernel times recorded since the previous report, as text lines "name\tms\tlaunches\n" (needs timing on);
 * a successful report clears the record. */
cl_status cl_ctx_kernel_times(cl_ctx* ctx, char* buf, uint64_t cap, uint64_t* needed);
/* Enable/disable per-kernel HIP-event timing (off by default; on adds event records around kernels). */
void cl_ctx_set_timing(cl_ctx* ctx, int on);
/* Opt-in check of the edit scripts (off by default; with it off nothing below is launched and every output byte is the same).
 * While it is on, cl_compress_shard on this context and a cl_compressor created on it (which hands the flag to its encode lanes)
 * rebuild every read of every chunk on the device from its own edit script and the reference reads (cl_es_verify) right after
 * cl_encode_reads, and compare it with the input, before the streams are coded: a read that differs makes the call return
 * CL_E_MISMATCH, the text naming the chunk-relative read and its first differing base.  The entropy-coded bytes are not decoded.
 * cl_ctx_verified: reads and bases checked so far on this context and its compressor's lanes. */
void cl_ctx_set_verify(cl_ctx* ctx, int on);
cl_status cl_ctx_verified(const cl_ctx* ctx, uint64_t* reads, uint64_t* bases);
/* Opt-in check of the entropy-coded bytes (off by default; with it off nothing below is launched or allocated and every output byte
 * is the same).  While it is on, cl_dna_encode and cl_qual_encode on this context (and so cl_compress_shard and a cl_compressor
 * created on it, which hands the flag to its quality coder's context) run every coded part, in its final place in the caller's
 * buffer, through the DECODER's interval arithmetic on the device (CRangeDecoder, sub_rc.h:216-392: Start, GetCumulativeFreq,
 * UpdateFrequency with its renormalisation), one lane per part: every symbol must fall in the interval (cum, freq, total) its model
 * gave it, and the part must end at its size (8 + the bytes the renormalisation asks for).  A part that does not: CL_E_MISMATCH, the
 * text naming the stream, the part in call order, its symbols and bytes and the first symbol that does not decode (or the bytes
 * consumed and stored).  Together with cl_ctx_set_verify: input -> edit scripts and triples -> final bytes are covered.  NOT
 * covered: edit scripts -> sort keys -> triples — the models themselves are not replayed (walks, sorts, model evolution).  A quality
 * coder of mode `none` codes nothing and checks nothing.
 * cl_ctx_verified_streams: parts, symbols and bytes the coders have checked so far ON THIS CONTEXT (a quality coder with a context of
 * its own counts there; cl_compressor_verified_streams adds them up). */
void cl_ctx_set_verify_streams(cl_ctx* ctx, int on);
cl_status cl_ctx_verified_streams(const cl_ctx* ctx, uint64_t* parts, uint64_t* symbols, uint64_t* bytes);
/* Which aligner took the gaps of the LAST cl_encode_reads on this context, summed over its recursion levels (host counts the call
 * keeps anyway: no launch, no allocation).  Writes min(cap, 11) values: out[0..7] gaps per size class (0 trivial, 1..4 small with that
 * many 64-row blocks, 5 four per wave, 6 a wave each, 7 giant: tile jobs), out[8] class-5 gaps the wave kernel redid (distance beyond
 * the band), out[9] giant gaps the tile jobs handed back to the wave kernel, out[10] further rounds of the wave kernel with larger
 * pools.  COLORD_HIP_GAP_DEBUG prints the same per level. */
cl_status cl_ctx_gap_paths(const cl_ctx* ctx, uint64_t* out, uint32_t cap);
/* Content digest: reads and symbols counted, and a 64-bit sum over the reads that depends on every symbol, on its place
 * in its read and on the read's index g in the whole input — and on nothing else (not on parts, chunks, lanes, domains or ranks).
 * Digests of disjoint sets of reads add field by field (wrapping), in any order. */
typedef struct cl_digest { uint64_t reads, symbols, sum; } cl_digest;
/* Opt-in digests of the input (off by default; with it off nothing below is launched or allocated and every output byte is the
 * same).  While it is on, cl_compress_shard on this context (its reads are reads 0 .. n-1) and cl_compressor_encode of a
 * cl_compressor created on it (every chunk, at its global read index, on this context, before the coders start) add the digests of
 * the chunk's bases (cl_digest_bases) and, with a quality stream, of its quality symbols (cl_digest_quals) to the context's totals.
 * They are taken from the input arena and the input quality bytes only, never from anything the encoder made.
 * cl_ctx_digest: the totals so far (either pointer may be null). */
void cl_ctx_set_digest(cl_ctx* ctx, int on);
cl_status cl_ctx_digest(const cl_ctx* ctx, cl_digest* dna, cl_digest* qual);
/* Opt-in digest of the quality VALUES (off by default: one flag test, no launch, no allocation, every output byte the same; a flag
 * of its own, independent of cl_ctx_set_digest).  While it is on, the same calls add, next to the other two and before the coders
 * start, the qual-values digest of the chunk (cl_digest_qual_values) at its global read index to the context's total — nothing
 * without a quality stream or in mode none.  The quality parameters must carry the -D values (rev) for *-fix: CL_E_INVALID if not.
 * cl_ctx_digest_values: the total so far. */
void cl_ctx_set_digest_values(cl_ctx* ctx, int on);
cl_status cl_ctx_digest_values(const cl_ctx* ctx, cl_digest* out);

/* ---- read arena: replaces read_t / read_pack_t (src/colord/utils.h:366-376, in_reads.cpp:24-42) -- */
/* d_codes: concatenated bases, 1 byte per base; either codes 0..4 (ascii=0) or ASCII ACGTN, upper
 * case only as the reference (ascii=1; anything else: CL_E_INVALID "Only ACGTN symbols supported inside a read").  d_offsets: n_reads+1 base offsets into d_codes.  Builds the 2-bit arena: every read starts
 * on a 32-base (uint64) word boundary and is followed by at least one pad base; a parallel bit mask
 * marks N and pad bases invalid. */
cl_status cl_reads_pack(cl_ctx* ctx, const uint8_t* d_codes, const uint64_t* d_offsets, uint32_t n_reads,
                        int ascii, cl_reads** out);
void cl_reads_free(cl_reads* r);
uint32_t cl_reads_count(const cl_reads* r);
uint64_t cl_reads_total_bases(const cl_reads* r);
uint64_t cl_reads_total_words(const cl_reads* r);
const uint64_t* cl_reads_packed(const cl_reads* r);     /* device: words, base j of a word in bits 63-2j..62-2j */
const uint32_t* cl_reads_invalid(const cl_reads* r);    /* device: per word, bit 31-j set = base j is N/pad */
const uint64_t* cl_reads_word_offsets(const cl_reads* r); /* device: n_reads+1 */
const uint32_t* cl_reads_lengths(const cl_reads* r);    /* device: n_reads */
const uint8_t* cl_reads_has_n(const cl_reads* r);       /* device: n_reads (1 = read contains N) */

/* ---- a1: CKmerWalker + CHashModuloFilter (in_reads.h:30-74, filtering-KMC/hash_filter.h:8-77) ---- */
/* Pass-1 scan: every N-free k-window of every read, canonical form, kept iff fmix64(kmer) % f == 0.
 * Survivors are written unordered to d_out (capacity cap, in k-mers); *n_out = number produced
 * (CL_E_CAPACITY if > cap; then only the first cap were written). */
cl_status cl_kmer_scan(cl_ctx* ctx, const cl_reads* reads, uint32_t k, uint32_t f,
                       uint64_t* d_out, uint64_t cap, uint64_t* n_out);

/* ---- a2 + a3: run_filtering_kmc + CKmerFilter (filtering_kmc.h:5-18, count_kmers.cpp:57-93,
 *      kmer_filter.h:30-167, filter_kmers.cpp:45-93) --------------------------------------------- */
typedef struct {
	uint64_t n_reads;              /* "#Total_reads" (caller-supplied read count is echoed) */
	uint64_t tot_kmers;            /* "#Total no. of k-mers" */
	uint64_t n_unique;             /* "#Unique_k-mers" */
	uint64_t n_unique_counted;     /* "#Unique_counted_k-mers" */
	uint64_t total_count_filtered; /* CKmerFilter::GetTotalKmers() */
} cl_kmer_stats;
/* d_kmers (n survivors of cl_kmer_scan, possibly from several arenas) is sorted in place; distinct
 * k-mers with multiplicity >= ci are kept with counter min(count, cs).  Builds the membership table.
 * Any n: above 2^30 k-mers the input is counted key range by key range (d_kmers is then left unsorted). */
cl_status cl_kmer_count_filter(cl_ctx* ctx, uint64_t* d_kmers, uint64_t n, uint32_t k, uint32_t ci, uint32_t cs,
                               cl_kmer_set** out, cl_kmer_stats* stats);
/* Set object from keys that are already counted/filtered (ascending, distinct) — used to replicate the
 * set on every GPU after the all-gather of the per-rank key partitions (SURVEY §8e exchange 1). */
cl_status cl_kmer_set_create(cl_ctx* ctx, const uint64_t* d_keys, const uint32_t* d_counts, uint64_t n, uint32_t k, cl_kmer_set** out);
void cl_kmer_set_free(cl_kmer_set* s);
uint64_t cl_kmer_set_size(const cl_kmer_set* s);
const uint64_t* cl_kmer_set_keys(const cl_kmer_set* s);   /* device, ascending */
const uint32_t* cl_kmer_set_counts(const cl_kmer_set* s); /* device, saturated counters */
/* CKmerFilter::Check for a batch of k-mers: d_found[i] = 1/0 */
cl_status cl_kmer_set_check(cl_ctx* ctx, const cl_kmer_set* s, const uint64_t* d_kmers, uint64_t n, uint8_t* d_found);

/* ---- a4: CReadsSimilarityGraph::getAcceptedKmers (reads_sim_graph.cpp:128-169, 221-228) ---------- */
/* Per read without N and with len >= k: the distinct canonical k-mers that pass the modulo test and
 * are in the set, in first-occurrence order. */
cl_status cl_accepted_kmers(cl_ctx* ctx, const cl_kmer_set* set, const cl_reads* reads, uint32_t k, uint32_t f,
                            cl_kmer_lists** out);
void cl_kmer_lists_free(cl_kmer_lists* l);
uint32_t cl_kmer_lists_reads(const cl_kmer_lists* l);
uint64_t cl_kmer_lists_total(const cl_kmer_lists* l);
const uint64_t* cl_kmer_lists_offsets(const cl_kmer_lists* l); /* device, n_reads+1 */
const uint64_t* cl_kmer_lists_kmers(const cl_kmer_lists* l);   /* device, k-mer values */
const uint32_t* cl_kmer_lists_ids(const cl_kmer_lists* l);     /* device, rank of each k-mer in the set */
const uint32_t* cl_kmer_lists_pos(const cl_kmer_lists* l);     /* device, start position in the read */

/* ---- a6: CRefReadsAccepter (ref_reads_accepter.h:23-58) ------------------------------------------ */
/* Host function (one sequential mt19937 stream, negligible cost).  h_out[i], i < n_pseudo + n_reads. */
cl_status cl_ref_accept(uint32_t n_reads, uint32_t n_pseudo, uint32_t range, double exponent, uint8_t* h_out);

/* ---- a5: CKmersToReads + processReadsPack[HiFi] (reads_sim_graph.h:45-119, .cpp:295-528) --------- */
/* d_accept[i] (n_reads bytes): read i becomes a reference read (acceptor decision AND no N).  The first
 * n_pseudo reads of `lists` are reference-genome pseudo reads (always accepted, list cap not applied).
 * Builds, for every k-mer of the set, the list of the first max_kmer_count reference ids containing it. */
cl_status cl_index_build(cl_ctx* ctx, const cl_kmer_set* set, const cl_kmer_lists* lists, const uint8_t* d_accept,
                         uint32_t n_pseudo, uint32_t max_kmer_count, cl_index** out);
/* Multi-GPU form of the same build (SURVEY §8e exchange 2).  cl_index_entries_of lists the (k-mer id,
 * reference id) pairs of this rank's accepted reads in read order, reference ids starting at ref_base;
 * d_bounds (n_reads+1, optional) receives ref_base + number of accepted reads before each local read.
 * After an all-gather in rank order the concatenated pairs (ascending reference id) go to
 * cl_index_build_pairs, which sorts d_ids/d_refs in place. */
cl_status cl_index_entries_of(cl_ctx* ctx, const cl_kmer_lists* lists, const uint8_t* d_accept, uint32_t ref_base,
                              uint32_t* d_ids, uint32_t* d_refs, uint64_t cap, uint64_t* n_out,
                              uint32_t* d_bounds, uint32_t* n_accepted);
cl_status cl_index_build_pairs(cl_ctx* ctx, const cl_kmer_set* set, uint32_t* d_ids, uint32_t* d_refs, uint64_t n,
                               const uint32_t* d_bounds, uint32_t n_reads, uint32_t n_refs_total,
                               uint32_t n_pseudo, uint32_t max_kmer_count, cl_index** out);
void cl_index_free(cl_index* ix);
uint32_t cl_index_n_refs(const cl_index* ix);
uint64_t cl_index_entries(const cl_index* ix);
const uint32_t* cl_index_ref_rank(const cl_index* ix);   /* device, n_reads+1: #references before read i */
/* For every read i: up to max_candidates earlier reference reads sharing most accepted k-mers, ordered
 * by (votes desc, ref id asc).  d_refs / d_votes: n_reads * max_candidates (row-major, unused = ~0u / 0),
 * d_n: n_reads. */
cl_status cl_candidates(cl_ctx* ctx, const cl_index* ix, const cl_kmer_lists* lists, uint32_t max_candidates,
                        uint32_t* d_refs, uint32_t* d_votes, uint32_t* d_n);
/* The same query for one CHUNK of reads against an index built over the reference reads of the WHOLE input
 * (cl_index_build_pairs with n_reads = 0): d_bounds[i] = number of reference reads that precede read i in file order. */
cl_status cl_candidates_at(cl_ctx* ctx, const cl_index* ix, const cl_kmer_lists* lists, const uint32_t* d_bounds, uint32_t max_candidates,
                           uint32_t* d_refs, uint32_t* d_votes, uint32_t* d_n);
/* HiFi variant (processReadsPackHiFi): additionally, per chosen candidate, the shared k-mers in read
 * order.  d_common_off: n_reads*max_candidates+1 offsets into d_common (capacity cap k-mers);
 * *n_common = needed size. */
cl_status cl_candidates_common(cl_ctx* ctx, const cl_index* ix, const cl_kmer_lists* lists, uint32_t max_candidates,
                               const uint32_t* d_refs, const uint32_t* d_n,
                               uint64_t* d_common_off, uint64_t* d_common, uint64_t cap, uint64_t* n_common);

/* ---- a13 + a15 + a16: CQualityCoder / CEntrComprQuals (quality_coder.{h,cpp}, quality_coder_impl.cpp,
 *      entr_qual.h:100-135; range coder sub_rc.h:44-212; models rc.h) ---------------------------------- */
typedef struct cl_qual_coder cl_qual_coder;
typedef struct {
	int32_t mode;        /* QualityComprMode (params.h:33-43): 0 org, 1 5-avg, 2 4-avg, 3 2-avg, 4 5-fix, 5 4-fix, 6 2-fix, 7 avg, 8 none */
	int32_t source;      /* DataSource: 0 ONT, 1 PBRaw, 2 PBHiFi */
	int32_t level;       /* compression level 1..3 */
	uint32_t n_fwd;      /* -T thresholds (bins - 1 values) */
	uint32_t fwd[8];
	uint32_t n_rev;      /* -D representatives (decoder side only; carried for completeness) */
	uint32_t rev[8];
} cl_qual_params;
/* CQualityCoder::Init(true, ...): one adaptive model set that persists across cl_qual_encode calls. */
cl_status cl_qual_coder_create(cl_ctx* ctx, const cl_qual_params* params, cl_qual_coder** out);
void cl_qual_coder_free(cl_qual_coder* q);
cl_ctx* cl_qual_coder_ctx(const cl_qual_coder* q);          /* the context the coder was created on */
/* CEntrComprQuals::Compress for a batch of whole parts.  Reads [h_part_bounds[p], h_part_bounds[p+1]) of the
 * arena form part p (the reference cuts parts where sum(len+1) >= 4 Mi, in_reads.cpp:62-77; any cut at read
 * boundaries yields a valid archive).  d_quals: ASCII quality bytes, d_qual_off: n_reads+1 offsets into it
 * (read i has the same length as in the arena).  d_flags (level > 1 only, else NULL): per-base class bytes
 * 'A' / 'M' / other (quality_coder_impl.cpp:25-75), same offsets.  Output: part payloads back to back in
 * d_out (capacity cap), h_part_sizes[n_parts]; *n_out = total bytes. */
cl_status cl_qual_encode(cl_ctx* ctx, cl_qual_coder* q, const cl_reads* reads, const uint8_t* d_quals, const uint64_t* d_qual_off,
                         const uint8_t* d_flags, const uint32_t* h_part_bounds, uint32_t n_parts,
                         uint8_t* d_out, uint64_t cap, uint64_t* h_part_sizes, uint64_t* n_out);

/* Model domains of the quality stream (no counterpart in the reference, whose one model set lives for the whole file, entr_qual.h:100-135,
 * and whose decoder is therefore one dependent chain, entr_qual.h:136-260).  n = 0 (the default): none — every byte and every launch as
 * without this call.  While n > 0 the coder starts a new domain at the first part boundary at which the symbols coded since the open
 * domain's start (per-base symbols and average bytes) have reached n: both model families go back to their initial state, exactly a
 * fresh coder's, behind the evolution of the last part before.  A domain is a whole number of parts; the first starts with the coder.
 * The parts of a domain are byte for byte those of a fresh cl_qual_coder given the domain's reads alone.  CL_E_INVALID while a batch is
 * prepared or evolved ahead (cl_compressor_prepare_parts).  The reference's decompressor cannot read such a stream: it carries its
 * models on (quality_coder.cpp:605-657); cl_qual_decoder_new_domain / cl_qual_decode_domains read it.
 * cl_qual_coder_domains: the first part of every domain so far (parts counted over the coder's lifetime; the first entry is 0);
 * *n_out = their number, CL_E_CAPACITY if it exceeds cap (nothing is written then). */
cl_status cl_qual_coder_set_domain_symbols(cl_qual_coder* q, uint64_t n);
cl_status cl_qual_coder_domains(const cl_qual_coder* q, uint64_t* h_first_part, uint64_t cap, uint64_t* n_out);
/* Test access: out[0 .. n_sym) = the counters and out[n_sym] = the total of one adaptive model as the last finished cl_qual_encode left
 * them (all ones before its first symbol); *n_out = n_sym + 1, CL_E_CAPACITY if that exceeds cap.
 * family 0, the per-base models (2, 4, 5 or 96 symbols): the context by its components, never by the library's private id —
 *   bits 0-23   the history fields, four bits each, the field of the position before in bits 0-3: the symbol coded there (org: its
 *               quantised class), 0xF where the read has no such position; fields the mode does not have are 0
 *   bits 32-39  the bases b0 (this position, bits 32-33), bm1, bm2 (the one and two before, 0 where there is none), bp1 (the one
 *               behind, 0 at the read's end), N as A; bit 40: the position is the read's third or a later one
 *   bits 48-49  levels 2 and 3: 1 = unit match ('M'), 2 = inside an anchor ('A')
 * family 1, the 256-symbol models of the average bytes: context = bin * 128 + floor(average of the bin before) for a high byte
 * (avg: 0), 640 + high byte for a low byte.
 * Waits for the context's stream and the coder's own; CL_E_INVALID for an unknown family or context, or while a batch is prepared or
 * evolved ahead.
 * cl_qual_coder_groups: the groups of parts the coder has taken through its model kernels so far (one per call unless a call holds a
 * domain start or more symbols than a group may: 2^31 - 2^24, or COLORD_HIP_QUAL_GROUP_SYMS, read per call, which changes no byte). */
cl_status cl_qual_coder_model(const cl_qual_coder* q, uint32_t family, uint64_t context, uint32_t* out, uint32_t cap, uint32_t* n_out);
cl_status cl_qual_coder_groups(const cl_qual_coder* q, uint64_t* n_out);

/* ---- a8: m-mer anchors (encoder.cpp:291-493,617-776,1016-1111,1149-1192,1577-1622) ------------------------ */
typedef struct cl_anchors cl_anchors;
/* prepareEncodeCandidates + fixOverlaping* for every read of `reads` (non-HiFi path): for each of its <= c candidate
 * reference ids (d_cand_refs row-major n_reads*c, d_cand_n per read — the output of cl_candidates; ids index `refs`,
 * the arena of reference reads) both orientations are analysed: shared m-mers (m = anchor_len, not canonical), "too
 * many matches" veto, LIS chain, merge into anchors; the better orientation is kept (reverse complement wins ties),
 * candidates are sorted by total anchor length (stable) and overlaps trimmed.  Reads with N, shorter than m or with
 * too few distinct m-mers get no candidates (they are stored plain). */
cl_status cl_anchor_candidates(cl_ctx* ctx, const cl_reads* reads, const cl_reads* refs, const uint32_t* d_cand_refs, const uint32_t* d_cand_n,
                               uint32_t c, uint32_t anchor_len, double frac_always, double frac_min, double max_matches_mult,
                               uint32_t min_anchors, cl_anchors** out);
/* a9, DataSource::PBHiFi (prepareEncodeCandidatesHiFi, KmerBasedAnchors, AnalyseRefReadWithKmers; encoder.cpp:870-1013,
 * 1113-1147,1194-1253): as above, but a candidate is first anchored on the k-mers it shares with the read
 * (d_common_off / d_common from cl_candidates_common; kmer_len, modulo = the graph's k and f): k-mers unique in both
 * reads seed anchors of length k, which must be colinear, are extended base by base and merged; the m-mer analysis
 * decides only the candidates without accepted k-mer anchors. */
cl_status cl_anchor_candidates_hifi(cl_ctx* ctx, const cl_reads* reads, const cl_reads* refs, const uint32_t* d_cand_refs, const uint32_t* d_cand_n,
                                    uint32_t c, uint32_t anchor_len, double frac_always, double frac_min, double max_matches_mult,
                                    uint32_t min_anchors, uint32_t kmer_len, uint32_t modulo, const uint64_t* d_common_off, const uint64_t* d_common,
                                    cl_anchors** out);
void cl_anchors_free(cl_anchors* a);
uint64_t cl_anchors_total(const cl_anchors* a);
/* how the call chained its (read, candidate, orientation) tasks: non-empty tasks and their match pairs that went through the
   wave form (tasks of at least COLORD_HIP_LIS_WAVE_MIN pairs) and through the lane form; counted on the device */
uint64_t cl_anchors_wave_tasks(const cl_anchors* a);
uint64_t cl_anchors_wave_pairs(const cl_anchors* a);
uint64_t cl_anchors_lane_tasks(const cl_anchors* a);
uint64_t cl_anchors_lane_pairs(const cl_anchors* a);
const uint32_t* cl_anchors_n_cands(const cl_anchors* a);        /* device, n_reads */
const uint32_t* cl_anchors_cands(const cl_anchors* a);          /* device, n_reads*c*4: ref_id, rev, tot_anchor_len, n_anchors */
const uint64_t* cl_anchors_cand_offsets(const cl_anchors* a);   /* device, n_reads*c+1: first anchor of each slot */
const uint32_t* cl_anchors_data(const cl_anchors* a);           /* device, 3 per anchor: len, pos_in_enc, pos_in_ref */

/* ---- a12 (plain forms): CEncoder::AddPlainRead / AddPlainReadWithN (encoder.cpp:663-681) --------------- */
/* Tuple streams that store every read of the arena verbatim: `start_plain` (`start_plain_with_Ns` for reads
 * containing N) + one `plain` tuple per base.  d_es needs total_bases + n_reads bytes (cap), d_es_off
 * n_reads+1, d_es_ntuples n_reads.  This is what the reference emits for a read without usable candidates. */
cl_status cl_encode_plain(cl_ctx* ctx, const cl_reads* reads, uint8_t* d_es, uint64_t cap, uint64_t* d_es_off,
                          uint32_t* d_es_ntuples, uint64_t* n_out);

/* ---- a10 + a11 + a12: CEncoder::Encode (encoder.cpp:1672-1691) on anchored candidates ------------------- */
/* Every read of `reads` is encoded against its candidates from cl_anchor_candidates (same arena, same c):
 * gaps between anchors are aligned with edlib's observable behaviour (edit_script.h:156-419), indels canonicalised
 * (refactor_edit_script), each gap kept as edit script or replaced by literals / an alternative reference
 * (EncodePart, EncodeWithAlternativeRead up to max_rec levels), and the result written as es_t tuple bytes
 * (utils.h:56-273).  h_pack_bounds (n_packs+1 read indices, first 0, last n_reads) are the reader packs: the
 * adaptive cost estimator (CEntropyEstimator, utils.h:877-1130) is reset at each of them (encoder.cpp:1677).
 * Reads without candidates and reads with N are stored plain.  d_es (cap bytes) receives the streams back to back,
 * d_es_off n_reads+1 byte offsets, d_es_ntuples n_reads tuple counts; *n_out = bytes needed (CL_E_CAPACITY if > cap). */
cl_status cl_encode_reads(cl_ctx* ctx, const cl_reads* reads, const cl_reads* refs, const cl_anchors* anchors, uint32_t c, uint32_t anchor_len,
                          uint32_t min_part_alt, uint32_t max_rec, double cost_mult, const uint32_t* h_pack_bounds, uint32_t n_packs,
                          uint8_t* d_es, uint64_t cap, uint64_t* d_es_off, uint32_t* d_es_ntuples, uint64_t* n_out);

/* The logarithm every cost decision of the encoder is made of, evaluated ON THE DEVICE exactly as the decision kernels do:
 * d_out[i] = d_count[i] ? -log2((double)d_count[i] * (1.0 / d_total[i])) : 0.0  (calc_logs, utils.h:800-810; the entropy of
 * CEntropy, utils.h:706-757, takes log2 of the same products).  The sums built from these values are plain IEEE additions
 * and multiplications (the library is compiled without FMA contraction), so pinning this function against the host's libm
 * over the reachable (count, total) pairs pins the decisions (tests/test_gpu_floatpin.py). */
cl_status cl_estimator_logs(cl_ctx* ctx, const uint32_t* d_count, const uint32_t* d_total, uint64_t n, double* d_out);

/* The per-base classes the quality coder uses at levels 2 and 3 (analyze_es, quality_coder_impl.cpp:25-75), from the
 * reads' own tuple streams: 'P' plain read, 'A' base inside an anchor tuple, 'M' unit match, ' ' inserted or substituted.
 * d_base_off: n_reads+1 offsets of the reads' bases (the d_qual_off of cl_qual_encode); d_flags: total_bases bytes. */
cl_status cl_es_flags(cl_ctx* ctx, const cl_reads* reads, const uint8_t* d_es, const uint64_t* d_es_off, const uint64_t* d_base_off, uint8_t* d_flags);

/* ---- the inverse of a10-a12: a read from its tuple stream, as CDNACoder::Decode applies the tuples it decoded
 *      (dna_coder.cpp:234-437) to what CEncoder::Encode wrote (encoder.cpp:1672-1691) — on the device, a wave per read ---------- */
/* The reads that the tuple streams d_es / d_es_off (n_reads + 1 byte offsets) describe against the reference arena `refs`: base
 * codes 0..4, one byte per base, back to back in d_codes (capacity cap) — the input form of cl_reads_pack with ascii = 0 — and
 * their n_reads + 1 offsets in d_base_off; *n_out = bases (CL_E_CAPACITY with the size needed if > cap; the offsets are valid then).
 * d_es_ntuples (optional): the tuple counts the streams must have.  A malformed stream (unknown or truncated tuple, id or position
 * outside the references, more than 64 alternatives, other tuple count) is CL_E_INVALID, the text naming the first such read; it
 * never makes the kernels read or write out of range. */
cl_status cl_es_expand(cl_ctx* ctx, const cl_reads* refs, const uint8_t* d_es, const uint64_t* d_es_off, const uint32_t* d_es_ntuples, uint32_t n_reads,
                       uint8_t* d_codes, uint64_t cap, uint64_t* d_base_off, uint64_t* n_out);
/* The same walk compared with the arena `reads` the streams were made from instead of stored (nothing is written but the counts):
 * *n_bad = reads whose length, tuple count or any base (N included) differs, *first_bad = the first of them (~0u: none).  CL_OK
 * with the counts; a malformed stream is CL_E_INVALID as above. */
cl_status cl_es_verify(cl_ctx* ctx, const cl_reads* reads, const cl_reads* refs, const uint8_t* d_es, const uint64_t* d_es_off, const uint32_t* d_es_ntuples,
                       uint64_t* n_bad, uint32_t* first_bad);

/* ---- content digests (no counterpart in the reference: its format has no checksum) — on the device, a wave per read ------------- */
/* The dna digest of every read of the arena, read i being read first_read + i of the input (first_read + n_reads <= 2^63), added to
 * *acc (host).  A read's words: per 32-base block the arena's packed word and its invalid mask, everything at or behind the read's
 * end cleared and the packed bits under an N forced to 0; n = bases. */
cl_status cl_digest_bases(cl_ctx* ctx, const cl_reads* reads, uint64_t first_read, cl_digest* acc);
/* The qual digest: per read the symbols the quality coder of `qparams` codes for it, in coding order, as bytes, eight to a word
 * little-endian — org and *-fix: map_fwd[q - 33] per base; *-avg: the 2 x bins average bytes, then the per-base bin symbols; avg: its
 * two average bytes; none: nothing at all (*acc is left as it is).  d_quals / d_qual_off as for cl_qual_encode; nothing outside
 * [d_qual_off[r], d_qual_off[r + 1]) is read for read r. */
cl_status cl_digest_quals(cl_ctx* ctx, const cl_qual_params* qparams, const cl_reads* reads, const uint8_t* d_quals, const uint64_t* d_qual_off,
                          uint64_t first_read, cl_digest* acc);
/* The same digests on the HOST, for what a decoder returns.  cl_digest_bases_host: h_codes as cl_dna_decode_part writes them (low
 * three bits the code, 4 = N; flag bits ignored), h_off n + 1 offsets.  cl_digest_bytes_host: kind 1 dna / 2 qual / 3 header; read i
 * = the bytes [h_off[i], h_off[i + 1]) of h_bytes (ids followed by their '+' byte; explicit symbol sequences). */
cl_status cl_digest_bases_host(const uint8_t* h_codes, const uint64_t* h_off, uint64_t n, uint64_t first_read, cl_digest* acc);
cl_status cl_digest_bytes_host(uint32_t kind, const uint8_t* h_bytes, const uint64_t* h_off, uint64_t n, uint64_t first_read, cl_digest* acc);
/* The qual-values digest (kind 4): what the quality DECODER will write for the reads, stated from the input qualities.  Per read one
 * byte per base in read order, the decoded value minus 33, eight to a word little-endian; n = bases.  With q = input byte - 33
 * (outside 0..95: 0) and bin = the bin of q under the -T thresholds — org: q; *-fix: rev[bin], the -D values
 * (quality_coder_impl.cpp:313-435); *-avg and avg (one bin): the k-th base of a bin in the read gets
 * floor(k A / 256) - floor((k - 1) A / 256), A = the bin's two average bytes as one integer — the decoders' error diffusion
 * `as += avg; v = (uint32)(as - qs); qs += v` (quality_coder_impl.cpp:506-559,800-849; CQualityCoder's decode, quality_coder.cpp:605-657),
 * exact in IEEE double because every partial sum is a multiple of 1/256; none: nothing at all (*acc is left as it is).  CL_E_INVALID:
 * thresholds that do not fit the mode, *-fix without a -D value for every bin, a -D value above 222.  Nothing outside
 * [d_qual_off[r], d_qual_off[r + 1]) is read for read r. */
cl_status cl_digest_qual_values(cl_ctx* ctx, const cl_qual_params* qparams, const cl_reads* reads, const uint8_t* d_quals, const uint64_t* d_qual_off,
                                uint64_t first_read, cl_digest* acc);
/* The values themselves: d_values[d_qual_off[r] + i] = the ASCII byte (value + 33) the decoder will write for base i of read r; nothing
 * outside [d_qual_off[r], d_qual_off[r + 1]) is written for read r.  cap: the bytes of d_values (CL_E_CAPACITY below the last offset,
 * d_qual_off[n_reads], before anything is launched).  Mode none: CL_E_INVALID. */
cl_status cl_qual_values(cl_ctx* ctx, const cl_qual_params* qparams, const cl_reads* reads, const uint8_t* d_quals, const uint64_t* d_qual_off,
                         uint8_t* d_values, uint64_t cap);
/* On the HOST.  cl_qual_values_host: the same values from input qualities (read i = [h_off[i], h_off[i + 1]) of h_quals) into h_values
 * at the same offsets.  cl_digest_qual_values_host: the qual-values digest of DECODED quality lines (ASCII, as a decoder returns
 * them), read i being read first_read + i of the input, added to *acc. */
cl_status cl_qual_values_host(const cl_qual_params* qparams, const uint8_t* h_quals, const uint64_t* h_off, uint64_t n, uint8_t* h_values);
cl_status cl_digest_qual_values_host(const uint8_t* h_ascii_quals, const uint64_t* h_off, uint64_t n, uint64_t first_read, cl_digest* acc);

/* ---- content report (no counterpart in the reference) — what the input holds and what the quality mode changes ------ */
/* Every counter is unsigned 64-bit and adds over disjoint sets of reads, in any order; len_min / len_max combine by min / max
 * (len_min is UINT64_MAX while reads == 0) and has_qual by or.  base_count: A, C, G, T, N (N = every position of a read whose bit is
 * set in the arena's invalid mask; pad positions are no content).  len_hist / len_bases: reads, and their bases, by bit length of the
 * read length (length 0 in bin 0).  The quality part (all zero and has_qual 0 for FASTA input and mode none): mean_q_hist per read of
 * length > 0 floor(sum q / len) of the INPUT qualities, q = byte - 33, outside 0..95 counted as 0 — the arithmetic mean of the Phred
 * values, not the error-probability mean; q_joint[in][out] = bases whose input quality is `in` and whose decoded quality value (the
 * byte the decoder WRITES minus 33: the quantity of the qual-values digest) is `out`. */
typedef struct cl_report {
	uint64_t reads, bases, base_count[5], len_min, len_max, len_hist[33], len_bases[33];
	uint64_t has_qual, q_reads, q_symbols, mean_q_hist[96], q_joint[96][96];
} cl_report;
void cl_report_clear(cl_report* r);
void cl_report_add(cl_report* dst, const cl_report* src);
/* On the device, added to *acc (host).  cl_report_bases: the content part of the arena, a wave per read, popcounts on the packed
 * words and the invalid mask.  cl_report_quals: the quality part, persistent blocks of four waves that count every byte into a
 * 96 x 96 matrix of 32-bit cells in LDS and add its non-zero cells to the 64-bit total at their end and whenever flush_bytes bytes
 * or more were counted since the last time (0: the default, 2^30; clamped to 1 .. 2^32 - 2^16); max_blocks: the grid's bound (0: the
 * default, four per CU).  Both arguments change no result.  d_quals / d_qual_off as for cl_qual_encode; nothing outside
 * [d_qual_off[r], d_qual_off[r + 1]) is read for read r.  Mode none: nothing is added.  CL_E_INVALID before any launch: thresholds
 * that do not fit the mode, a *-fix mode without a -D value for every bin or with one above 95.  CL_E_UNSUPPORTED: four consecutive
 * reads of 2^32 or more quality bytes together (a 32-bit cell could wrap). */
cl_status cl_report_bases(cl_ctx* ctx, const cl_reads* reads, cl_report* acc);
cl_status cl_report_quals(cl_ctx* ctx, const cl_qual_params* qparams, const cl_reads* reads, const uint8_t* d_quals, const uint64_t* d_qual_off,
                          uint64_t flush_bytes, uint32_t max_blocks, cl_report* acc);
/* On the HOST.  cl_report_bases_host: codes as cl_dna_decode_part writes them.  cl_report_quals_host: from INPUT quality bytes, as
 * the device.  cl_report_values_host: from DECODED quality lines (ASCII) — q_reads, q_symbols and the OUT marginal alone: every base
 * is counted in q_joint[0][out], so only the column sums of such a report mean anything. */
cl_status cl_report_bases_host(const uint8_t* h_codes, const uint64_t* h_off, uint64_t n, cl_report* acc);
cl_status cl_report_quals_host(const cl_qual_params* qparams, const uint8_t* h_ascii_quals_in, const uint64_t* h_off, uint64_t n, cl_report* acc);
cl_status cl_report_values_host(const uint8_t* h_ascii_values_out, const uint64_t* h_off, uint64_t n, cl_report* acc);
/* Opt-in (off by default: one flag test per chunk, no launch, no allocation, every output byte the same).  While it is on,
 * cl_compress_shard on this context and cl_compressor_encode of a compressor created on it add the report of every chunk's input —
 * the arena and, with a quality stream, the input quality bytes — to the context's total, before the coders start.
 * cl_ctx_report: the total so far (cleared when the flag is switched on). */
void cl_ctx_set_report(cl_ctx* ctx, int on);
cl_status cl_ctx_report(const cl_ctx* ctx, cl_report* out);

/* ---- edit-operation profile (no counterpart in the reference) — what the compressor did with the bases -------------- */
/* Counted from the tuple streams of a batch (the output of cl_encode_reads) and the reference reads they point to.  THIS IS THE
 * DIVERGENCE BETWEEN A READ AND THE REFERENCE READS IT WAS CODED AGAINST — earlier reads of the same input, and both carry
 * sequencing errors.  It is NOT a per-read error rate, except against the pseudo reads of a reference genome (-G); and it covers
 * only what the encoder aligned: reads coded plain, and the stretches an edit script skips, say nothing.
 * Every counter is unsigned 64-bit and adds over disjoint sets of reads, in any order.
 *   reads, bases            all reads of the batch and the bases their streams produce
 *   kind_reads / kind_bases / kind_bytes [3]   reads, bases and stream bytes by first tuple: 0 start-plain, 1 start-plain-with-Ns,
 *                           2 start-es (an edit script)
 *   main_rev[2]             edit-script reads by the orientation nibble of their start-es tuple (0, not 0)
 *   tuples[8]               tuples inside edit scripts by type 0..7: ins, del, match, subst, anchor, skip, alt-id, main-ref (the start
 *                           tuple is not counted)
 *   anchor_bases, anchor_len_hist[29]   sum of the anchor lengths; anchors by bit length of the length (0 -> 0, 1 -> 1, 2..3 -> 2, ..)
 *   skip_entries, skip_entry_sum        skips whose preceding tuple in the stream is an alt-id: their value is the position at which the
 *                           alternative is entered, not bases passed over
 *   skip_bases, skip_len_hist[29]       every other skip: the sum of the values, and the skips by bit length of the value
 *   ins_base[4]             inserted bases
 *   del_base[4], match_base[4]          the reference base under the cursor, in the read's orientation (complemented on a reversed
 *                           reference)
 *   sub[from][to]           from = the reference base under the cursor, to = the read's base; the diagonal is 0
 *   ins_run_hist[17], del_run_hist[17]  maximal runs of consecutive ins (del) tuples in one read's stream — any other tuple and the
 *                           stream's end close a run — by min(length, 16); index 0 stays 0
 *   identity_hist[101], identity_none   per edit-script read, m = matches + anchor bases, d = m + subst + ins + del: the read counts in
 *                           bin floor(100 m / d), or in identity_none when d = 0
 *   alt_hist[65]            edit-script reads by the number of DISTINCT alternative reference ids they use (0..64) */
typedef struct cl_edits {
	uint64_t reads, bases, kind_reads[3], kind_bases[3], kind_bytes[3], main_rev[2], tuples[8];
	uint64_t anchor_bases, anchor_len_hist[29], skip_entries, skip_entry_sum, skip_bases, skip_len_hist[29];
	uint64_t ins_base[4], del_base[4], match_base[4], sub[4][4], ins_run_hist[17], del_run_hist[17];
	uint64_t identity_hist[101], identity_none, alt_hist[65];
} cl_edits;
void cl_edits_clear(cl_edits* e);
void cl_edits_add(cl_edits* dst, const cl_edits* src);
/* The profile of n_reads tuple streams (d_es / d_es_off: n_reads + 1 byte offsets, as cl_encode_reads writes them) against the arena
 * `refs`, added to *acc (host).  On the device, a wave per read, the stream 64 bytes per step; anchors are not copied, so a read costs
 * its stream bytes / 64 and one reference base per del, match or subst tuple.  Persistent blocks of four waves count into 32-bit
 * cells in LDS, which are added to the 64-bit total at a block's end and whenever flush_bytes stream bytes or more were counted since
 * the last time (0: the default, 2^30; clamped to 1 .. 2^32 - 2^16); max_blocks: the grid's bound (0: the default, four per CU).
 * Both arguments change no result.  A malformed stream (empty, a bad first tuple, a type not allowed inside a script, a tuple that
 * crosses the stream's end, an id or position outside the references, a base value out of range, a 65th alternative) is
 * CL_E_INVALID, the text naming the first such read, and NOTHING of the batch is added; it never makes the kernel read out of range.
 * CL_E_UNSUPPORTED: four consecutive reads of 2^32 or more stream bytes together (a 32-bit cell could wrap). */
cl_status cl_edit_profile(cl_ctx* ctx, const cl_reads* refs, const uint8_t* d_es, const uint64_t* d_es_off, uint32_t n_reads,
                          uint64_t flush_bytes, uint32_t max_blocks, cl_edits* acc);
/* The same on the HOST, a sequential walk with the same checks and the same answers: reference read i = the base codes 0..3 at
 * [h_ref_off[i], h_ref_off[i + 1]) of h_ref_codes.  bad_read / bad_code (optional): the first malformed read and what it ran into
 * (cl_edit_profile_error names the code). */
cl_status cl_edit_profile_host(const uint8_t* h_ref_codes, const uint64_t* h_ref_off, uint32_t n_refs, const uint8_t* h_es, const uint64_t* h_es_off,
                               uint64_t n_reads, cl_edits* acc, uint64_t* bad_read, uint32_t* bad_code);
const char* cl_edit_profile_error(uint32_t code);
/* Opt-in (off by default: one flag test per batch, no launch, no allocation, every output byte the same).  While it is on, every
 * batch of tuple streams made on this context — by cl_compress_shard, by cl_compressor_encode, or by an encode lane of a compressor
 * created on it — adds its profile.  cl_ctx_edit_profile: the total so far of this context and its compressor's lanes (cleared when
 * the flag is switched on). */
void cl_ctx_set_edit_profile(cl_ctx* ctx, int on);
cl_status cl_ctx_edit_profile(const cl_ctx* ctx, cl_edits* out);

/* ---- k-mer count spectrum (no counterpart in the reference) — what the k-mer stage saw -------------------------------- */
/* How many distinct sampled k-mers occur once, twice, and so on: the run lengths of the sorted keys of cl_kmer_count_filter, BEFORE
 * the cut at ci and the saturation at cs.  The k-mers are the 1-in-f hash sample of cl_kmer_scan, so every number is of the sample.
 * Every field is unsigned 64-bit and adds over disjoint key ranges, in any order, except max_count, which combines by max.
 *   kmers        occurrences counted: the sum of c over all distinct k-mers (= cl_kmer_stats.tot_kmers)
 *   distinct     distinct k-mers (= cl_kmer_stats.n_unique)
 *   max_count    the largest c
 *   exact[c]     distinct k-mers that occur exactly c times, 1 <= c <= 4095; exact[0] stays 0
 *   big[b], big_mass[b]   k-mers with c >= 4096 by the bit length b of c (13..32): how many, and the sum of their c */
#define CL_KSPEC_EXACT 4096
typedef struct cl_kspec {
	uint64_t kmers, distinct, max_count;
	uint64_t exact[CL_KSPEC_EXACT];
	uint64_t big[33], big_mass[33];
} cl_kspec;
void cl_kspec_clear(cl_kspec* s);
void cl_kspec_add(cl_kspec* dst, const cl_kspec* src);
/* The spectrum of the runs of a sorted key array of n keys (n < 2^32), added to *acc (host): d_head_pos[0 .. n_heads) holds the
 * ascending start positions of the runs, run j has (j + 1 < n_heads ? d_head_pos[j + 1] : n) - d_head_pos[j] keys.  On the device
 * (k_run_spectrum): persistent blocks of 256 lanes count into 32-bit cells in LDS, the values 1..8 per wave by ballot, and add the
 * non-zero cells to a 64-bit scratch total at their end; max_blocks bounds the grid (0: the default, four per CU) and changes no
 * result.  Positions that are not strictly ascending or not below n, n_heads > n and n >= 2^32 are CL_E_INVALID and NOTHING is
 * added; they never make the kernel read or count out of range.  n_heads == 0 is CL_OK and adds nothing. */
cl_status cl_kmer_spectrum_heads(cl_ctx* ctx, const uint32_t* d_head_pos, uint64_t n_heads, uint64_t n, uint32_t max_blocks, cl_kspec* acc);
/* Opt-in (off by default: one flag test per counted key range, no launch, no allocation, every output the same).  While it is on,
 * every cl_kmer_count_filter on this context — the one-sort path and every key range above the count limit; in a multi-GPU run a
 * rank's own key range — adds the spectrum of what it counted.  cl_ctx_kmer_spectrum: the total so far (cleared when the flag is
 * switched on). */
void cl_ctx_set_kmer_spectrum(cl_ctx* ctx, int on);
cl_status cl_ctx_kmer_spectrum(const cl_ctx* ctx, cl_kspec* out);

/* ---- k-mer MinHash sketch (no counterpart in the reference) — is this archive the same sample as that one? ------------- */
/* Of the distinct sampled k-mers that occur at least min_count times (the runs of the sorted keys of cl_kmer_count_filter with that
 * many keys), the `size` smallest values of cl_sketch_hash(kmer), each with the k-mer's count: a bottom-s MinHash sketch.
 *   cl_sketch_hash(x) = fmix64(x ^ 0x9E3779B97F4A7C15), fmix64 being the finaliser of MurmurHash3 that the sampling test of
 *   cl_kmer_scan uses on x itself (fmix64(x) % f == 0); the xor decouples the two.  fmix64 is a bijection of the 64-bit words: two
 *   different k-mers never share a hash, and a k-mer can be recovered from its entry.  The same function runs on the device.
 * The k-mers are the 1-in-f hash sample of cl_kmer_scan: sketches made with the same k and f have sampled the same sub-universe of
 * k-mers and compare; sketches of another k or f do not.  WHAT IT IS NOT: a sketch of an assembly — it is made of noisy reads, so a
 * distance from it is not comparable with Mash distances of genomes.
 * cl_sketch is a host-side accumulator: size (1 .. 2^20), min_count (>= 1), qualifying — the distinct k-mers with count >=
 * min_count, added over calls —, and n <= size entries strictly ascending by hash.  n < size means the sketch is COMPLETE: it holds
 * every qualifying k-mer.  MERGE RULE, used by every path: union by hash, the counts of equal hashes add, the lowest `size` stay;
 * qualifying adds.  That is exact over disjoint key ranges and ranks, where no hash can repeat.  It is exact for independent k-mer
 * sets too (a hash in the union's bottom-`size` is in the bottom-`size` of every set that holds it, so its summed count is
 * complete); min_count then applies PER SET and qualifying is a sum over the sets, which counts a k-mer once per set that holds it. */
#define CL_SKETCH_MAX_SIZE (1u << 20)
typedef struct cl_sketch_entry { uint64_t hash, count; } cl_sketch_entry;
typedef struct cl_sketch cl_sketch;
uint64_t cl_sketch_hash(uint64_t kmer);
/* An empty accumulator with these parameters (any values: the calls that fill it refuse size 0, size > 2^20 and min_count 0). */
cl_status cl_sketch_create(uint32_t size, uint32_t min_count, cl_sketch** out);
void cl_sketch_free(cl_sketch* s);
/* what it holds (any pointer may be NULL); its entries, ascending, into h_out (cap < n: CL_E_CAPACITY, nothing written) */
cl_status cl_sketch_info(const cl_sketch* s, uint32_t* size, uint32_t* min_count, uint64_t* qualifying, uint64_t* n);
cl_status cl_sketch_entries(const cl_sketch* s, cl_sketch_entry* h_out, uint64_t cap);
/* The merge rule on the host: the n entries e (strictly ascending hashes, no count 0 — anything else is CL_E_INVALID and NOTHING is
 * merged) and `qualifying` into *dst. */
cl_status cl_sketch_merge(cl_sketch* dst, const cl_sketch_entry* e, uint64_t n, uint64_t qualifying);
/* The sketch of the runs of a sorted key array of n keys (n < 2^32), merged into *acc (host) with acc's size and min_count:
 * d_head_pos[0 .. n_heads) holds the ascending start positions of the runs (as cl_kmer_spectrum_heads), the key of run j is
 * d_keys[d_head_pos[j]].  On the device: k_sketch_bins counts the qualifying hashes in 4096 bins by their top 12 bits (LDS, then
 * 64-bit totals); the host takes the smallest bin B whose cumulative count reaches size; k_sketch_take writes the (hash, count)
 * pairs of the bins <= B — a block takes 4096 runs and ONE place in the output —, a radix sort orders them, and the first
 * min(size, candidates) come back.  max_blocks bounds both grids (0: the default, four per CU) and changes no result.
 * CL_E_INVALID, and NOTHING is merged: positions that are not strictly ascending or not below n (they never make a kernel read or
 * count out of range: a key is loaded at a validated position only), n_heads > n, n >= 2^32, acc's size 0 or above 2^20, acc's
 * min_count 0.  n_heads == 0 is CL_OK and merges nothing. */
cl_status cl_kmer_sketch_runs(cl_ctx* ctx, const uint64_t* d_keys, const uint32_t* d_head_pos, uint64_t n_heads, uint64_t n, uint32_t max_blocks, cl_sketch* acc);
/* Opt-in (off by default: one flag test per counted key range, no launch, no allocation, every output the same).  While it is on,
 * every cl_kmer_count_filter on this context — the one-sort path and every key range above the count limit; in a multi-GPU run a
 * rank's own key range — merges the sketch of what it counted.  Switching it on empties the context's sketch and sets its
 * parameters (size 0 or above 2^20, or min_count 0: CL_E_INVALID, the switch stays as it was).  cl_ctx_kmer_sketch: *out becomes a
 * copy of the context's sketch so far, parameters included (empty with size 0 if it was never switched on). */
cl_status cl_ctx_set_kmer_sketch(cl_ctx* ctx, int on, uint32_t size, uint32_t min_count);
cl_status cl_ctx_kmer_sketch(const cl_ctx* ctx, cl_sketch* out);

/* ---- read-to-read overlaps (no counterpart in the reference) — what the edit scripts aligned, per read ---------------- */
/* One record per VISIT of a read's tuple stream that holds an aligned column.  A visit is a stretch of tuples on one reference read:
 * it opens behind the start-es tuple and behind every alt-id / main-ref tuple; every alt-id and main-ref tuple closes the open one (a
 * main-ref met while on the main reference too), and so does the stream's end.  The walk is that of the edit profile with one more
 * cursor, the read position: ins read +1; del reference +1; match / subst both +1 (an aligned column); anchor v both +v (aligned iff
 * v > 0); skip v reference +v, the entry skip behind an alt-id included.  Plain reads and visits of insertions, deletions and skips
 * only give no record.  LIKE THE PROFILE THIS IS A READ AGAINST EARLIER READS, WHICH CARRY ERRORS OF THEIR OWN, and it lists overlaps
 * with REFERENCE reads only: about a tenth of the reads with the sparse acceptor, all of them otherwise.
 *   q               index of the read in the input
 *   t               the reference id as the stream has it, or the input index of that read where a translation table is given
 *   qlen, tlen      bases the stream produces; length of the reference read
 *   qs, qe          the read's interval: in front of the visit's first aligned column, behind its last (leading and trailing
 *                   insertions, deletions and skips do not count)
 *   ts, te          the same on the reference, in the reference's FORWARD coordinates (mirrored when it is taken reversed)
 *   matches         match tuples plus anchor lengths of the visit;  subst: its subst tuples;  anchor_bases: its anchor lengths
 *   flags           bit 0: the reference is taken reversed (an alternative's first appearance in the read decides);  bit 1: the main reference
 * The alignment block length is not stored: (qe - qs) + (te - ts) - matches - subst.  Records of a read are in visit order. */
typedef struct cl_overlap { uint32_t q, t, qlen, tlen, qs, qe, ts, te, matches, subst, anchor_bases, flags; } cl_overlap;
/* The records of n_reads tuple streams (d_es / d_es_off as cl_encode_reads writes them) against the arena `refs`, reads in order, into
 * d_out (device, cap records); read r of the batch is read first_read + r of the input.  d_ref_read (device, n_ref_read entries; or
 * null): reference id -> input index, for `t`; an id at or past n_ref_read is then malformed (a reference id outside).  On the device
 * (k_overlap_walk): a wave per read, the stream 64 bytes per step, persistent blocks of four waves (max_blocks bounds the grid, 0: four
 * per CU; it changes no result); one pass counts, a prefix sum places, the same kernel body fills.  *n_out = the records.  cap too
 * small (or d_out null): CL_E_CAPACITY, *n_out holds the need and nothing was written.  A malformed stream (the cases of
 * cl_edit_profile, and a read position past 2^32 - 1) is CL_E_INVALID, the text naming the first such read; *n_out = 0 and nothing is
 * handed out; it never makes the kernel read or write out of range. */
cl_status cl_overlaps_of(cl_ctx* ctx, const cl_reads* refs, const uint8_t* d_es, const uint64_t* d_es_off, uint32_t n_reads, uint64_t first_read,
                         const uint32_t* d_ref_read, uint32_t n_ref_read, uint32_t max_blocks, cl_overlap* d_out, uint64_t cap, uint64_t* n_out);
/* The same on the HOST (references as in cl_edit_profile_host), a sequential walk with the same checks in the same order; h_out may be
 * null to ask for the count.  bad_read / bad_code (optional): the first malformed read and its code (cl_edit_profile_error). */
cl_status cl_overlaps_host(const uint8_t* h_ref_codes, const uint64_t* h_ref_off, uint32_t n_refs, const uint8_t* h_es, const uint64_t* h_es_off, uint64_t n_reads,
                           uint64_t first_read, const uint32_t* h_ref_read, uint32_t n_ref_read, cl_overlap* h_out, uint64_t cap, uint64_t* n_out, uint64_t* bad_read, uint32_t* bad_code);
/* Opt-in (off by default: one flag test per batch, no launch, no allocation, every output byte the same).  While it is on, every batch
 * of tuple streams made on this context — by cl_compress_shard, by cl_compressor_encode, or by an encode lane of a compressor created on
 * it — leaves its records on the host, `t` translated to input indices.  cl_ctx_overlaps: those of this context and its compressor's
 * lanes so far, in input order (h_out, cap records; CL_E_CAPACITY with *n_out = the need and nothing written when cap is too small);
 * switching the flag on drops what was kept.  A compressor that shares its reads with other ranks, and the pseudo reads of a reference
 * genome, are refused while the flag is on (CL_E_UNSUPPORTED): their reference ids are not reads of this compressor's input. */
void cl_ctx_set_overlaps(cl_ctx* ctx, int on);
cl_status cl_ctx_overlaps(const cl_ctx* ctx, cl_overlap* h_out, uint64_t cap, uint64_t* n_out);

/* ---- read-to-genome mappings (no counterpart in the reference) — what a reference-genome run aligned, per read ------- */
/* With a reference genome the overlapping pieces of its sequences (the pseudo reads) are reference ids 0 .. n_pseudo-1, and a cl_overlap
 * whose `t` is such an id is an alignment of the read against a PIECE of the genome.  The LIFT moves it to the genome's sequences.
 * Geometry: n_seqs sequences of seq_len[s] bases, pieces of read_len bases every step = read_len - overlap bases; sequence s has
 * ceil(seq_len[s] / step) pieces (none when it has no base), piece p of it starts at p * step and is min(read_len, seq_len[s] - start)
 * long; the pieces of the sequences follow each other, so n_pseudo is their sum.  A record with t >= n_pseudo targets a read of the
 * input and is DROPPED; one with t < n_pseudo is kept: t = the sequence, tlen = its length, ts and te grow by the piece's start, flags
 * gets bit 2 (a target in genome coordinates), every other field stays.  The kept records stay in their order.
 * WHAT IT IS NOT: a read coded against earlier reads instead of genome pieces yields no record, and a read that spans a piece boundary
 * yields one record per piece; these are not stitched.
 * cl_mappings_lift: the n records at d_recs (device, at a multiple of 16 bytes, as cl_overlaps_of leaves them without a translation
 * table) into d_out (device, cap records); the geometry's lengths are on the host.  On the device (k_map_lift): a lane per record, one
 * pass flags, a prefix sum places, the same kernel body fills.  *n_out = the kept records.  cap too small (or d_out null):
 * CL_E_CAPACITY, *n_out holds the need and nothing was written.  A kept record whose tlen is not its piece's length (code 1), with a
 * lifted position past 2^32 - 1 (code 2) or with te lifted past the sequence's end (code 3) is CL_E_INVALID, the text naming the first
 * such record; *n_out = 0 and nothing is handed out.  read_len <= overlap is CL_E_INVALID; a sequence of 2^32 bases or more, and 2^32
 * pieces or records or more, CL_E_UNSUPPORTED. */
cl_status cl_mappings_lift(cl_ctx* ctx, const cl_overlap* d_recs, uint64_t n, const uint64_t* h_seq_len, uint32_t n_seqs, uint32_t read_len, uint32_t overlap,
                           cl_overlap* d_out, uint64_t cap, uint64_t* n_out);
/* The same on the HOST, the same checks in the same order; h_out may be null to ask for the count.  bad_record / bad_code (optional):
 * the first refused record and its code. */
cl_status cl_mappings_lift_host(const cl_overlap* h_recs, uint64_t n, const uint64_t* h_seq_len, uint32_t n_seqs, uint32_t read_len, uint32_t overlap,
                                cl_overlap* h_out, uint64_t cap, uint64_t* n_out, uint64_t* bad_record, uint32_t* bad_code);
/* Opt-in (off by default: one flag test per batch, no launch, no allocation, every output byte the same).  While it is on, every batch
 * of tuple streams made by cl_compressor_encode, or by an encode lane of a compressor created on this context, leaves its lifted records
 * on the host (the walk of cl_overlaps_of, then the lift).  cl_ctx_mappings: those of this context and its compressor's lanes so far, in
 * input order (h_out, cap records; CL_E_CAPACITY with *n_out = the need and nothing written when cap is too small); switching the flag
 * on drops what was kept.  cl_compressor_refs_finish refuses a compressor without pseudo reads or without their geometry
 * (cl_compressor_genome_geometry; CL_E_INVALID) and one that shares its reads with other ranks (CL_E_UNSUPPORTED); cl_compress_shard
 * has no pseudo reads and refuses the flag (CL_E_UNSUPPORTED).  Independent of cl_ctx_set_overlaps. */
void cl_ctx_set_mappings(cl_ctx* ctx, int on);
cl_status cl_ctx_mappings(const cl_ctx* ctx, cl_overlap* h_out, uint64_t cap, uint64_t* n_out);

/* ---- CIGARs (no counterpart in the reference) — the alignment of every overlap record, base by base ------------------- */
/* The CIGAR of a record (a VISIT of cl_overlaps_of that holds an aligned column) is the sequence of the operations of the visit's tuples
 * in stream order — ins: I 1; del: D 1; match: = 1; subst: X 1; anchor v: = v; skip v: D v (nothing for v = 0) — from the visit's first
 * aligned column to its last, both included: what lies in front of the first (the entry skip behind an alt-id too) and behind the last is
 * dropped, the trimming that qs / qe / ts / te do.  Neighbouring equal operations merge; a zero-length anchor or skip between them does
 * not keep them apart.  An operation is one uint32_t, len << 4 | op, with BAM's codes: I = 1, D = 2, = is 7, X = 8.  Operations are in
 * WALK order: the read forward, the reference in the orientation it is taken in; A RECORD WITH flags BIT 0 IS REVERSED BY WHOEVER PRINTS
 * IT (PAF and SAM have the target forward).  For every record: the lengths of = X I add up to qe - qs, those of = X D to te - ts, those of
 * = to matches, those of X to subst; the first and the last operation are = or X; no two neighbours are equal; every length is at least 1.
 * cl_cigars_of: the streams of cl_overlaps_of against the arena `refs`.  d_rec_ops (device, rec_cap words): the operation count of every
 * record, in the order of cl_overlaps_of's records (*n_rec of them); d_ops (device, ops_cap words): the operations of the records one
 * behind the other (*n_ops).  id_limit (0: every reference): a visit on a reference id at or past it gets the count 0 and no operation —
 * with id_limit = the pseudo reads of a genome the counts that are not 0 are those of the records cl_mappings_lift keeps, in their order.
 * On the device (k_cigar_walk): a wave per read as in cl_overlaps_of (max_blocks bounds the grid, 0: four per CU; it changes no result);
 * run heads from ballots, run lengths from a segmented wave sum; one pass counts, a prefix sum places, the same kernel body fills.
 * Either capacity too small (or its pointer null): CL_E_CAPACITY, both needs in *n_rec / *n_ops and nothing written.  A malformed stream
 * is CL_E_INVALID as in cl_overlaps_of; a merged run of 2^28 bases or more inside a record, and 2^32 records or more, CL_E_UNSUPPORTED,
 * the text naming the read; the counts are 0 then and nothing is handed out. */
cl_status cl_cigars_of(cl_ctx* ctx, const cl_reads* refs, const uint8_t* d_es, const uint64_t* d_es_off, uint32_t n_reads, uint32_t id_limit, uint32_t max_blocks,
                       uint32_t* d_rec_ops, uint64_t rec_cap, uint64_t* n_rec, uint32_t* d_ops, uint64_t ops_cap, uint64_t* n_ops);
/* The same on the HOST (references as in cl_edit_profile_host), a sequential walk with the same checks in the same order; the outputs may
 * be null to ask for the counts.  bad_read / bad_code (optional): the first refused read and its code — those of cl_overlaps_host, and
 * 256 for the run that does not fit (cl_cigars_error gives the text of either). */
cl_status cl_cigars_host(const uint8_t* h_ref_codes, const uint64_t* h_ref_off, uint32_t n_refs, const uint8_t* h_es, const uint64_t* h_es_off, uint64_t n_reads, uint32_t id_limit,
                         uint32_t* h_rec_ops, uint64_t rec_cap, uint64_t* n_rec, uint32_t* h_ops, uint64_t ops_cap, uint64_t* n_ops, uint64_t* bad_read, uint32_t* bad_code);
const char* cl_cigars_error(uint32_t code);
/* Opt-in (off by default: one flag test per batch, no launch, no allocation, every output byte the same), on top of cl_ctx_set_mappings:
 * while both are on, every batch leaves the CIGARs of its lifted records on the host too, made in the mappings' hook with the record
 * offsets of that batch's walk.  cl_ctx_cigars: those of this context and its compressor's lanes so far, in the order of cl_ctx_mappings'
 * records — a count per record and the operations (CL_E_CAPACITY with both needs and nothing written when a capacity is too small);
 * switching the flag on drops what was kept.  Switching it on without cl_ctx_set_mappings is CL_E_INVALID, and so is
 * cl_compressor_refs_finish when the mappings were switched off again; refused wherever the mappings are (ranks, cl_compress_shard). */
cl_status cl_ctx_set_cigars(cl_ctx* ctx, int on);
cl_status cl_ctx_cigars(const cl_ctx* ctx, uint32_t* h_rec_ops, uint64_t rec_cap, uint64_t* n_rec, uint32_t* h_ops, uint64_t ops_cap, uint64_t* n_ops);

/* ---- coded CIGARs (no counterpart in the reference) — the operations as the bytes of a static-model interval coder ----- */
/* An operation word len << 4 | op gives two symbols: the op symbol o (I 0, D 1, = 2, X 3), coded in the context of the o of the word
 * before it in flat order (context 4 at a part's first word), and the length symbol len - 1 for len <= 255, else 255 (escape: len follows
 * as a raw u32 in the segment's escape list), coded in the context of its own o.  The words of a call are cut into segments of seg_ops
 * (0: the default and maximum, 2^20), a segment into parts of part_ops (0: the default, 4096; at most 2^16); a part is one restart of the
 * interval coder.  The model is static per segment: the 20 + 1024 counts of its symbols are the frequencies.  Segment bytes, little-endian:
 * u32 n_ops, u32 part_ops, u32 n_escapes, u32 table_bytes; the part sizes as u32; the 1044 counts as LEB128; the escapes; the parts.
 * cl_cigars_pack: n_ops words in DEVICE memory (any sequence of words with an op of I D = X and len >= 1: record boundaries play no role)
 * -> the bytes of their segments in h_out (*n_bytes; 0 words give 0 bytes).  Histogram, model and interval coder run on the device; the
 * host copies the coded bytes.  cap too small (or h_out null): CL_E_CAPACITY with the need and nothing written.  Another word is
 * CL_E_INVALID, the text naming the first such index; a knob out of range too.  cl_cigars_pack_host: the same bytes from one host thread
 * (*bad_index, optional: the first word that is no operation, else ~0).  cl_cigars_unpack_host: the words back (*n_ops; CL_E_CAPACITY with
 * the need); bytes that are not whole segments of this format, in any way, are CL_E_INVALID and nothing outside them is read —
 * cl_cigars_check_host says why (0: they decode), cl_cigars_refusal gives the text. */
cl_status cl_cigars_pack(cl_ctx* ctx, const uint32_t* d_ops, uint64_t n_ops, uint32_t part_ops, uint32_t seg_ops, uint8_t* h_out, uint64_t cap, uint64_t* n_bytes);
cl_status cl_cigars_pack_host(const uint32_t* h_ops, uint64_t n_ops, uint32_t part_ops, uint32_t seg_ops, uint8_t* h_out, uint64_t cap, uint64_t* n_bytes, uint64_t* bad_index);
cl_status cl_cigars_unpack_host(const uint8_t* bytes, uint64_t n, uint32_t* h_ops, uint64_t cap, uint64_t* n_ops);
uint32_t cl_cigars_check_host(const uint8_t* bytes, uint64_t n);
const char* cl_cigars_refusal(uint32_t code);
/* Opt-in on top of cl_ctx_set_cigars (CL_E_INVALID without it; switching the CIGARs off switches this off): a batch's operations are coded
 * right after they are made and only the coded bytes come to the host.  cl_ctx_cigars decodes them there; cl_ctx_cigars_coded gives the
 * record counts (as cl_ctx_cigars) and the segments of all batches one behind the other, in the batches' order, with their operations and
 * segments counted (CL_E_CAPACITY with the needs and nothing written; CL_E_INVALID when a batch was kept raw).  Segment bytes depend on how
 * the input was batched; the decoded operations do not. */
cl_status cl_ctx_set_cigars_coded(cl_ctx* ctx, int on);
cl_status cl_ctx_cigars_coded(const cl_ctx* ctx, uint32_t* h_rec_ops, uint64_t rec_cap, uint64_t* n_rec, uint8_t* h_bytes, uint64_t cap, uint64_t* n_bytes, uint64_t* n_ops, uint64_t* n_segments);

/* ---- pileup (no counterpart in the reference) — what a reference-genome run aligned, per genome position ------------- */
/* The second half of what a -G run aligns: which genome position every read base was aligned to, and what the read said there.  The
 * geometry is that of cl_mappings_lift; the table has n_pos = sum of seq_len[s] positions, sequence s from the sum of the lengths before
 * it on.  A tuple met on reference id < n_pseudo, taken reversed or not, at cursor c of a piece of len bases that starts at table
 * position `origin` touches position origin + (rev ? len - 1 - c : c).  Tuples on an id >= n_pseudo (a read) count nothing; the walk, its
 * cursor and every check go on as in cl_edit_profile.  Per position eight 32-bit counters (cl_pileup_columns), which wrap at 2^32:
 *   match     match tuples and anchor bases
 *   sub[4]    subst tuples by the READ's base (A C G T) in the genome's FORWARD orientation (complemented when the piece is taken reversed)
 *   del       one per deleted reference base
 *   ins       one per insertion RUN — a maximal row of consecutive ins tuples in the stream; the start tuple, an alt-id and a main-ref
 *             end a row — booked at the forward position LEFT of it: cursor - 1 taken forward (none at cursor 0 or past the piece's
 *             end), len - 1 - cursor taken reversed (none at cursor >= len).  A run with no such position is counted in ins_unplaced only.
 *             (Unaligned read ends are coded as long insertion runs: per base they would bury the channel.)
 *   ref       the genome's base 0..3, filled by cl_pileup_finish
 * depth = match + sub + del.  An anchor of L > 0 bases is booked as a difference (+1 at its first position, -1 behind its last, modulo
 * 2^32) that cl_pileup_finish sums up into `match`.  Pieces overlap in the genome, so two pieces can reach one position; a read column
 * lies on one piece only, so nothing is counted twice.
 * WHAT IT IS NOT: reads coded against earlier reads instead of genome pieces count nothing; there are no per-strand counts; the
 * thresholds' defaults (4 / 3 / 250) are interface defaults, chosen so that isolated read errors do not qualify at ONT error rates, and
 * are not tuned against anything. */
typedef struct cl_pileup cl_pileup;
/* a site: its sequence and 0-based position in it, the genome's base, the channel that won (0..3 a base, 4 del, 5 ins), the counters */
typedef struct cl_pileup_site { uint32_t seq, pos, ref, kind, match, sub[4], del, ins, depth; } cl_pileup_site;
/* positions with depth >= 1; the sums of match, sub (all four), del and ins over the table; insertion runs without a position; the reads
 * of which a tuple (ins, del, match, subst, anchor or skip) was met on a genome piece */
typedef struct cl_pileup_sums { uint64_t covered, match, sub, del, ins, ins_unplaced, reads; } cl_pileup_sums;
/* The table for the genome whose pieces are reads 0 .. n_pseudo-1 of the arena `refs` (n_pseudo: the geometry's piece count), allocated
 * and zeroed: 36 bytes per position.  The piece count and every piece length are checked against the arena as
 * cl_compressor_genome_geometry checks them (CL_E_INVALID); read_len <= overlap is CL_E_INVALID; a sequence of 2^32 bases or more, 2^32
 * pieces or more and a table of 2^32 positions or more CL_E_UNSUPPORTED; an allocation that fails CL_E_NOMEM, the text giving the bytes
 * needed.  `refs` must stay alive and unchanged until cl_pileup_finish has run. */
cl_status cl_pileup_create(cl_ctx* ctx, const cl_reads* refs, const uint64_t* h_seq_len, uint32_t n_seqs, uint32_t read_len, uint32_t overlap, cl_pileup** out);
void cl_pileup_free(cl_pileup* p);
/* n_reads tuple streams (d_es / d_es_off as cl_encode_reads writes them) against `refs` — the arena given to cl_pileup_create, anything
 * else is CL_E_INVALID — added to the table.  On the device (k_pileup_walk): a wave per read, persistent blocks of four waves (max_blocks
 * bounds the grid, 0: four per CU; it changes no result), every tuple booked by its own lane with one device atomic, an anchor with two.
 * Safe from several threads at once on one object: the adds are device atomics on integers, and no result depends on their order.  A
 * malformed stream (the cases of cl_edit_profile) is CL_E_INVALID, the text naming the first such read; it never makes the kernel read
 * or write out of range, but the adds of the tuples before it cannot be taken back: the object is SPOILED, and every later call on it
 * but cl_pileup_free is refused (CL_E_INVALID). */
cl_status cl_pileup_add(cl_pileup* p, const cl_reads* refs, const uint8_t* d_es, const uint64_t* d_es_off, uint32_t n_reads, uint32_t max_blocks);
/* Once, after the last add (adds are refused afterwards, and so is a second finish: CL_E_INVALID): the anchors' running sum goes into
 * `match`, `ref` is filled from the pieces, the totals are summed (k_pileup_fold). */
cl_status cl_pileup_finish(cl_pileup* p);
/* after cl_pileup_finish.  The counters of positions first .. first + n - 1 of the table into h_out, 8 uint32 each: match, sub A C G T,
 * del, ins, ref (first + n > n_pos: CL_E_INVALID). */
cl_status cl_pileup_columns(const cl_pileup* p, uint64_t first, uint64_t n, uint32_t* h_out);
/* The sites in genome order into h_out (host, cap records): positions with depth >= min_depth whose ALT — the largest of sub[b] for
 * b != ref, del and ins, ties to the lowest kind — is >= min_alt and alt * 1000 >= min_permille * depth (k_pileup_sites: a lane per
 * position; one pass counts, a prefix sum places, the same kernel body fills).  *n_out = the sites.  cap too small (or h_out null):
 * CL_E_CAPACITY, *n_out holds the need and nothing was written. */
cl_status cl_pileup_sites(const cl_pileup* p, uint32_t min_depth, uint32_t min_alt, uint32_t min_permille, cl_pileup_site* h_out, uint64_t cap, uint64_t* n_out);
cl_status cl_pileup_totals(const cl_pileup* p, cl_pileup_sums* out);
uint64_t cl_pileup_positions(const cl_pileup* p);                                  /* n_pos */
/* The whole of it on the HOST (references as in cl_edit_profile_host, the first pieces of the geometry among them), a sequential walk
 * with the same checks in the same order: h_cols (n_pos x 8 uint32, or null), the sites (h_sites may be null to ask for the count;
 * CL_E_CAPACITY as above, h_cols and sums are written then too), sums.  bad_read / bad_code (optional): the first malformed read and its
 * code (cl_edit_profile_error); nothing is written then. */
cl_status cl_pileup_host(const uint8_t* h_ref_codes, const uint64_t* h_ref_off, uint32_t n_refs, const uint64_t* h_seq_len, uint32_t n_seqs, uint32_t read_len, uint32_t overlap,
                         const uint8_t* h_es, const uint64_t* h_es_off, uint64_t n_reads, uint32_t min_depth, uint32_t min_alt, uint32_t min_permille,
                         uint32_t* h_cols, cl_pileup_site* h_sites, uint64_t cap, uint64_t* n_sites, cl_pileup_sums* sums, uint64_t* bad_read, uint32_t* bad_code);
/* Opt-in (off by default: one flag test per batch, no launch, no allocation, every output byte the same).  While it is on, a compressor
 * created on this context makes ONE table in cl_compressor_refs_finish, from the geometry of cl_compressor_genome_geometry, and every
 * batch of tuple streams made by cl_compressor_encode or by one of its encode lanes is added to it.  cl_compressor_refs_finish refuses a
 * compressor without pseudo reads or without their geometry (CL_E_INVALID) and one that shares its reads with other ranks
 * (CL_E_UNSUPPORTED); cl_compress_shard has no pseudo reads and refuses the flag (CL_E_UNSUPPORTED).  Every model domain of the command
 * line is a compressor of its own, with a table of its own: the command line refuses --domains > 1.  Independent of the flags above. */
void cl_ctx_set_pileup(cl_ctx* ctx, int on);

/* ---- a14 + a16: CDNACoder / CEntrComprReads (dna_coder.{h,cpp}, entr_read.h:56-80) --------------------- */
typedef struct cl_dna_coder cl_dna_coder;
/* CDNACoder::Init(true, maxCandidates, level, ., n_ref_genome_pseudo_reads): one adaptive model set that
 * persists across cl_dna_encode calls; start_read_id seeds cur_read_id. */
cl_status cl_dna_coder_create(cl_ctx* ctx, uint32_t max_alt_refs, int32_t level, uint32_t start_read_id, cl_dna_coder** out);
void cl_dna_coder_free(cl_dna_coder* d);
/* Test access: out[0 .. n_sym) = the counters and out[n_sym] = the total of one adaptive model, as the last finished cl_dna_encode
 * left them (all ones before its first symbol).  family: 0 read type (3 symbols), 1 orientation (2), 2 seen (2), 3 length bits (32),
 * 4 length data (256), 5 symbols (4), 6 symbols with N (5), 7 read id (256), 8 short read id (max_alt_refs), 9 anchor length (24),
 * 10 local skip (256), 11 distant skip (256), 12 tuple type (8).  context: the reference's context value of that family where the
 * reference symbol is a base (positions past a reference read's end are kept apart).  A read-only copy after a wait for the
 * context's stream; CL_E_INVALID for an unknown family or context, or while a batch evolved ahead is held. */
cl_status cl_dna_coder_model(const cl_dna_coder* d, uint32_t family, uint64_t context, uint32_t* out);
/* CEntrComprReads::Compress for a batch of whole parts.  d_es: the reads' tuple streams (es_t byte layout,
 * utils.h:56-273) back to back, d_es_off: n_reads+1 byte offsets, d_es_ntuples: es_t::size() per read.
 * refs: arena whose read i is reference read i (CReferenceReads order).  Parts [h_part_bounds[p],
 * h_part_bounds[p+1]) must cover [0, n_reads).  Output as for cl_qual_encode; the archive metadata of
 * part p is its read count. */
cl_status cl_dna_encode(cl_ctx* ctx, cl_dna_coder* d, const cl_reads* refs, const uint8_t* d_es, const uint64_t* d_es_off,
                        const uint32_t* d_es_ntuples, uint32_t n_reads, const uint32_t* h_part_bounds, uint32_t n_parts,
                        uint8_t* d_out, uint64_t cap, uint64_t* h_part_sizes, uint64_t* n_out);

/* CReferenceReads (reference_reads.h:24-80): the arena of the reads with d_keep[i] != 0, in order — reference id r is
 * the r-th kept read.  The result is an independent arena (free with cl_reads_free). */
cl_status cl_reads_select(cl_ctx* ctx, const cl_reads* src, const uint8_t* d_keep, cl_reads** out);
/* An arena from words that already have the arena layout (word-aligned reads back to back; see cl_reads_packed /
 * cl_reads_invalid), e.g. the concatenation of the reference-read arenas of all ranks (the reference's
 * CReferenceReads is one process-wide store; with reads sharded over GPUs each rank replicates it). */
cl_status cl_reads_from_arena(cl_ctx* ctx, const uint64_t* d_packed, const uint32_t* d_inv, const uint32_t* d_lens, uint32_t n_reads, cl_reads** out);

/* ---- the `header` stream: CIDCoder + CEntrComprHeaders (id_coder.{h,cpp}, entr_header.cpp:23-45) — HOST functions --- */
typedef struct cl_id_coder cl_id_coder;
/* header_mode = HeaderComprMode (params.h:44): 0 Original (lossless), 1 Main, 2 None (the latter two code no id bytes,
 * as in the reference).  One coder per archive: models and the previous id persist from part to part. */
cl_status cl_id_coder_create(int32_t header_mode, cl_id_coder** out);
void cl_id_coder_free(cl_id_coder* c);
const char* cl_id_coder_error(const cl_id_coder* c);
/* One pack of headers -> one part (archive metadata = n).  h_ids: the ids back to back without the leading '@' / '>',
 * h_off: n+1 offsets, h_plus[i] != 0 when the '+' line of record i repeats the id.  The reference closes a pack when the
 * id bytes reach 4 Mi (in_reads.cpp:50-56,93-101).  cap >= 2 * id bytes + 64. */
cl_status cl_id_encode_part(cl_id_coder* c, const uint8_t* h_ids, const uint64_t* h_off, const uint8_t* h_plus, uint32_t n,
                            uint8_t* h_out, uint64_t cap, uint64_t* n_out);

/* ---- the whole compress data path of one shard: runCompression's stage wiring (compression.cpp:432-689) ---------- */
typedef struct {
	uint32_t k, f, ci, cs, c;                 /* kmerLen, filterHashModulo, minKmerCount, maxKmerCount, maxCandidates */
	uint32_t anchor_len, min_part_alt, max_rec, min_anchors;   /* anchorLen, minPartLenToConsiderAltRead, maxRecurence, minAnchors */
	int32_t level, source;                    /* compression level 1..3, DataSource (0 ONT, 1 PBRaw, 2 PBHiFi) */
	int32_t sparse;                           /* referenceReadsMode == Sparse (else every N-free read is a reference read) */
	double sparse_g, sparse_exponent;         /* sparseMode_range_symbols (in genome lengths), sparseMode_exponent */
	double cost_mult, frac_always, frac_min, max_matches_mult;   /* editScriptCostMultiplier, minFractionOfMmersInEncode*, maxMatchesMultiplier */
} cl_compress_params;
typedef struct {
	uint64_t n_reads, n_bases, tot_kmers, n_kept_kmers, n_refs, n_anchors, tuple_bytes, dna_bytes, qual_bytes;
	uint32_t sparse_range, pad;
} cl_compress_info;
/* reads (+ ASCII qualities d_quals with per-read offsets d_base_off, or NULLs with qual == NULL) -> `dna` and `qual` stream
 * parts.  h_part_bounds: the parts of both streams (read indices); h_pack_bounds: the reader packs (estimator reset).
 * dna / qual: the long-lived coders (model state persists across calls, as one CEntrCompr* thread).  Outputs as for
 * cl_dna_encode / cl_qual_encode.  If `qual` was created on a second context of the same GPU and level == 1 (no
 * dependence on the edit scripts) the quality stream is coded concurrently with the DNA path.  Single GPU; with reads sharded over GPUs the caller runs the stages itself around the
 * two exchanges (bench.py). */
cl_status cl_compress_shard(cl_ctx* ctx, const cl_compress_params* params, const cl_reads* reads, const uint8_t* d_quals, const uint64_t* d_base_off,
                            const uint32_t* h_part_bounds, uint32_t n_parts, const uint32_t* h_pack_bounds, uint32_t n_packs,
                            cl_dna_coder* dna, cl_qual_coder* qual,
                            uint8_t* d_dna_out, uint64_t dna_cap, uint64_t* h_dna_part_sizes,
                            uint8_t* d_qual_out, uint64_t qual_cap, uint64_t* h_qual_part_sizes, cl_compress_info* info);

/* ---- runCompression over an input of any size, chunk by chunk, on one GPU or on one GPU per rank --------------------
 * The reference streams the file twice: pass 1 counts the k-mers of the whole input (compression.cpp:432), pass 2 pushes
 * reader packs through graph -> encoder -> coders (compression.cpp:547-561, in_reads.cpp:62-77) while the similarity
 * graph grows (reads_sim_graph.cpp:324-427).  cl_compressor holds that state between calls.  A chunk is an arena of whole
 * reader packs (any size the GPU holds, e.g. 1 Gbase); the caller presents the same chunks, in file order, three times:
 *     cl_compressor_count_add (each chunk) -> cl_compressor_count_finish
 *     cl_compressor_refs_add  (each chunk) -> cl_compressor_refs_finish
 *     cl_compressor_encode    (each chunk)
 * The `dna` / `qual` parts are byte-identical to one cl_compress_shard call over the whole input.
 *
 * cl_exchange: with reads sharded over GPUs (one process per GPU, rank r holds the r-th contiguous range of the file)
 * the two *_finish steps exchange what SURVEY.md section 8e lists: k-mers go to the rank owning their key range and the
 * kept keys are all-gathered (replicated set); reference reads and index entries are all-gathered (replicated store and
 * index).  The caller supplies the collectives (colord_amd/parallel.py: torch.distributed, "nccl" = RCCL over xGMI);
 * every rank must call the compressor functions in the same order.  Each rank is its own model domain of the coders. */
typedef struct cl_compressor cl_compressor;
typedef struct {
	void* user;
	uint32_t rank, world;
	/* host: every rank contributes n uint64; h_out[world * n] receives them in rank order */
	cl_status (*all_gather_host)(void* user, const uint64_t* h_vals, uint32_t n, uint64_t* h_out);
	/* device: d_send holds the bytes for rank 0, 1, ... back to back (h_send_bytes[world]); d_recv receives the bytes
	 * from rank 0, 1, ... back to back (h_recv_bytes[world]) */
	cl_status (*all_to_all_v)(void* user, const void* d_send, const uint64_t* h_send_bytes, void* d_recv, const uint64_t* h_recv_bytes);
	/* device: d_recv = the send buffers of rank 0, 1, ... back to back; h_recv_bytes[world] (send_bytes == h_recv_bytes[rank]) */
	cl_status (*all_gather_v)(void* user, const void* d_send, uint64_t send_bytes, void* d_recv, const uint64_t* h_recv_bytes);
} cl_exchange;
/* qual_ctx: second context of the same GPU for the quality stream (coded concurrently at level 1), or NULL.  qparams NULL =
 * no quality stream.  exchange NULL = single GPU.  expected_bases: size hint for the k-mer buffer of pass 1 (0 = unknown). */
cl_status cl_compressor_create(cl_ctx* ctx, cl_ctx* qual_ctx, const cl_compress_params* params, const cl_qual_params* qparams,
                               const cl_exchange* exchange, uint64_t expected_bases, cl_compressor** out);
void cl_compressor_free(cl_compressor* c);
cl_status cl_compressor_count_add(cl_compressor* c, const cl_reads* chunk);
/* stats (optional): the statistics over the whole input (all ranks) */
cl_status cl_compressor_count_finish(cl_compressor* c, cl_kmer_stats* stats);
cl_status cl_compressor_refs_add(cl_compressor* c, const cl_reads* chunk);
cl_status cl_compressor_refs_finish(cl_compressor* c);
/* arguments as for cl_compress_shard, bounds relative to the chunk */
cl_status cl_compressor_encode(cl_compressor* c, const cl_reads* chunk, const uint8_t* d_quals, const uint64_t* d_base_off,
                               const uint32_t* h_part_bounds, uint32_t n_parts, const uint32_t* h_pack_bounds, uint32_t n_packs,
                               uint8_t* d_dna_out, uint64_t dna_cap, uint64_t* h_dna_part_sizes,
                               uint8_t* d_qual_out, uint64_t qual_cap, uint64_t* h_qual_part_sizes, cl_compress_info* info);
/* Reference-genome mode (`-G`; compression.cpp:405-447, reference_genome.cpp:372-429, reads_sim_graph.cpp:295-322).  With reads
 * sharded over GPUs every rank makes both calls with the SAME sequences / pseudo reads: rank 0 counts the genome's k-mers and
 * contributes the pseudo reads to the replicated reference store, the other ranks only take note of their number:
 *   cl_compressor_genome_add    before count_finish: the genome's sequences (arenas of ACGT codes, any number of calls) are a second
 *                               input of the k-mer counter; the statistics of count_finish are corrected for them as in the reference;
 *   cl_compressor_pseudo_reads  once, after count_finish and before the first refs_add: the overlapping pieces of the sequences
 *                               (length 20 x mean_read_len of cl_compressor_info, overlap 10 x (k - 1)) become reference reads
 *                               0 .. n-1 — always accepted, their k-mer lists uncapped; the acceptor and the DNA coder count them. */
cl_status cl_compressor_genome_add(cl_compressor* c, const cl_reads* sequences);
cl_status cl_compressor_pseudo_reads(cl_compressor* c, const cl_reads* pseudo_reads);
/* Optional look-ahead of pass 2.  Announces a chunk that a LATER cl_compressor_encode call will present (announce in file
 * order, before the chunk is encoded; the arena and the bounds' meaning stay as they are until that call returns).  What the
 * chunk needs before the coders — a4 accepted k-mers, a5 candidates, a8/a9 anchors, a10-a12 edit scripts and tuple streams —
 * depends on no earlier chunk's output (the reference's graph and encoder threads run ahead of its two coder threads in the
 * same way, compression.cpp:547-661), so it is computed in the background on a context of the compressor's own ("encode
 * lane", COLORD_HIP_ENCODE_LANES of them, default 2, each with its own HIP streams and memory pool, about 30 GB per 1-Gbase chunk) while the caller's
 * thread codes the chunks before it; only the adaptive models of the `dna` / `qual` coders chain chunk to chunk.  The lanes
 * run at most lanes + 2 chunks ahead of the encode calls.  Output bytes are the same with or without announcements. */
cl_status cl_compressor_prepare(cl_compressor* c, const cl_reads* chunk, const uint32_t* h_pack_bounds, uint32_t n_packs);
/* The same with the coder parts the chunk will be encoded with (h_part_bounds of the later cl_compressor_encode call): then the half
 * of the `dna` coder that needs no model state — tuple walks, triple slots, the stable sort by (family, context), context runs;
 * the reference's CEntrComprReads thread does all of that inline, entr_read.h:56-80 — is made ahead as well, on a preparation
 * thread and context of the compressor's own, one or two chunks ahead of the encode calls (~15 GB per 1-Gbase chunk ahead); the
 * caller's stream keeps model evolution and interval coding.  Announcements must start with the first chunk.  With d_quals /
 * d_base_off (those of the later encode call; null: not prepared) the same for the `qual` coder at level 1: symbols, sort by
 * context and context runs on a second preparation thread (~8 GB per 1-Gbase chunk ahead).  Bytes unchanged.  The announcement is
 * BINDING while the compressor evolves ahead (long parts, mean >= 2^19 symbols, or COLORD_HIP_EVOLVE_DEPTH > 0): the adaptive models
 * of the next chunks are then advanced from the announced bounds and quality buffer before their encode call and cannot be rolled
 * back — an encode call with other part bounds or buffers fails with CL_E_INVALID ("the batch evolved ahead is not the one encoded
 * next") and the compressor is unusable afterwards.  Without evolve-ahead a differing encode call is honoured (the preparation is
 * redone). */
cl_status cl_compressor_prepare_parts(cl_compressor* c, const cl_reads* chunk, const uint32_t* h_pack_bounds, uint32_t n_packs, const uint32_t* h_part_bounds, uint32_t n_parts,
                                      const uint8_t* d_quals, const uint64_t* d_base_off);
/* what the archive's `meta` stream needs (compression.cpp:704-779), valid after count_finish (n_refs_total after refs_finish):
 * first_read = global index of this rank's first read (start of its model domain) */
cl_status cl_compressor_info(const cl_compressor* c, cl_kmer_stats* stats, uint64_t* first_read, uint64_t* n_reads_total, uint64_t* mean_read_len,
                             uint32_t* sparse_range, uint32_t* n_refs_total);
/* cl_ctx_verified of the compressor's context: the reads and bases its encode calls and lanes have checked (cl_ctx_set_verify) */
cl_status cl_compressor_verified(const cl_compressor* c, uint64_t* reads, uint64_t* bases);
/* cl_ctx_verified_streams summed over the contexts that code for the compressor (its own and its quality coder's): the parts, symbols
 * and bytes of the dna and qual streams that were decoded against their models' intervals (cl_ctx_set_verify_streams) */
cl_status cl_compressor_verified_streams(const cl_compressor* c, uint64_t* parts, uint64_t* symbols, uint64_t* bytes);
/* cl_ctx_digest of the compressor's context: the digests of the chunks encoded so far (cl_ctx_set_digest); read indices are global:
 * this rank's first read (cl_compressor_info) + the reads of its chunks before */
cl_status cl_compressor_digest(const cl_compressor* c, cl_digest* dna, cl_digest* qual);
/* cl_ctx_digest_values of the compressor's context (cl_ctx_set_digest_values) */
cl_status cl_compressor_digest_values(const cl_compressor* c, cl_digest* out);
/* cl_ctx_report of the compressor's context (cl_ctx_set_report): the report of the chunks encoded so far */
cl_status cl_compressor_report(const cl_compressor* c, cl_report* out);
/* cl_ctx_edit_profile of the compressor's context (cl_ctx_set_edit_profile): the profile of the chunks whose tuple streams are made,
 * its encode lanes' included — after the last cl_compressor_encode, of every chunk */
cl_status cl_compressor_edit_profile(const cl_compressor* c, cl_edits* out);
/* cl_ctx_kmer_spectrum of the compressor's context (cl_ctx_set_kmer_spectrum): after cl_compressor_count_finish, the spectrum of the
 * k-mers pass 1 counted (a reference genome's included) */
cl_status cl_compressor_kmer_spectrum(const cl_compressor* c, cl_kspec* out);
/* cl_ctx_kmer_sketch of the compressor's context (cl_ctx_set_kmer_sketch): after cl_compressor_count_finish, the sketch of the k-mers
 * pass 1 counted (a reference genome's included); in a multi-GPU run of the key range this rank owns */
cl_status cl_compressor_kmer_sketch(const cl_compressor* c, cl_sketch* out);
/* cl_ctx_overlaps of the compressor's context (cl_ctx_set_overlaps): after the last cl_compressor_encode, of every chunk */
cl_status cl_compressor_overlaps(const cl_compressor* c, cl_overlap* h_out, uint64_t cap, uint64_t* n_out);
/* The geometry of the pseudo reads (cl_mappings_lift), for cl_ctx_set_mappings: once, behind cl_compressor_pseudo_reads and before
 * cl_compressor_refs_finish.  The piece count and every piece length are made again from it; a geometry that does not give the
 * compressor's n_pseudo pseudo reads with exactly their lengths is refused (CL_E_INVALID).  The tables stay on the device. */
cl_status cl_compressor_genome_geometry(cl_compressor* c, const uint64_t* h_seq_len, uint32_t n_seqs, uint32_t read_len, uint32_t overlap);
/* cl_ctx_mappings of the compressor's context (cl_ctx_set_mappings): after the last cl_compressor_encode, of every chunk */
cl_status cl_compressor_mappings(const cl_compressor* c, cl_overlap* h_out, uint64_t cap, uint64_t* n_out);
/* cl_ctx_cigars of the compressor's context (cl_ctx_set_cigars): after the last cl_compressor_encode, of every chunk */
cl_status cl_compressor_cigars(const cl_compressor* c, uint32_t* h_rec_ops, uint64_t rec_cap, uint64_t* n_rec, uint32_t* h_ops, uint64_t ops_cap, uint64_t* n_ops);
/* cl_ctx_cigars_coded of the compressor's context (cl_ctx_set_cigars_coded) */
cl_status cl_compressor_cigars_coded(const cl_compressor* c, uint32_t* h_rec_ops, uint64_t rec_cap, uint64_t* n_rec, uint8_t* h_bytes, uint64_t cap, uint64_t* n_bytes, uint64_t* n_ops, uint64_t* n_segments);
/* The compressor's table (cl_ctx_set_pileup), finished, after the last cl_compressor_encode: *out belongs to the compressor and goes
 * with it.  CL_E_INVALID: the flag was off when the references were finished, or chunks are still to be coded. */
cl_status cl_compressor_pileup(cl_compressor* c, cl_pileup** out);

/* cl_qual_coder_set_domain_symbols / cl_qual_coder_domains of the compressor's quality coder.  The setting must be made before the
 * first cl_compressor_encode or cl_compressor_prepare_parts call (CL_E_INVALID afterwards, and without a quality stream); the `dna`
 * coder is not touched.  The domains are valid after cl_compressor_refs_finish. */
cl_status cl_compressor_set_qual_domain_symbols(cl_compressor* c, uint64_t n);
cl_status cl_compressor_qual_domains(const cl_compressor* c, uint64_t* h_first_part, uint64_t cap, uint64_t* n_out);

/* ---- a17, the inverse path: CRangeDecoder (sub_rc.h:216-392), CDNACoder::Decode (dna_coder.cpp:234-437), CQualityCoder::Decode
 *      (quality_coder.cpp:605-657, quality_coder_impl.cpp:506-559,800-849), CIDCoder::Decode (id_coder.cpp:396-600); drivers
 *      CEntropyDecomprReads / CEntrDecomprQuals / CEntrDecomprHeaders (entr_read.h:146-191, entr_qual.h:136-260, entr_header.cpp:46-80).
 *      HOST functions (h_* pointers): a model domain decodes as one dependent chain; streams and domains are the parallelism. ---- */
/* The `ref-genome` stream of archives written with -G -s (CReferenceGenome::Store / its archive constructor,
 * reference_genome.cpp:235-279,325-370): every sequence a plain read under the DNA coder's "level 9" models, one part whose
 * archive metadata is the number of sequences.  h_codes: bases 0..3 back to back, h_off: n_seqs + 1 offsets.  HOST functions.
 * CL_E_CAPACITY with *n_out = bytes needed when the output does not fit. */
cl_status cl_genome_encode(const uint8_t* h_codes, const uint64_t* h_off, uint32_t n_seqs, uint8_t* h_out, uint64_t cap, uint64_t* n_out);
cl_status cl_genome_decode(const uint8_t* h_in, uint64_t n_in, uint32_t n_seqs, uint8_t* h_codes, uint64_t cap, uint64_t* h_off, uint64_t* n_out);
/* MD5 of the sequences in the reference's packed form — what the `meta` stream carries instead of the genome without -s
 * (reference_genome.cpp:29-67,205-213; compression.cpp:771-776). */
cl_status cl_genome_md5(const uint8_t* h_codes, const uint64_t* h_off, uint32_t n_seqs, uint8_t* h_md5_16);

typedef struct cl_dna_decoder cl_dna_decoder;
typedef struct cl_qual_decoder cl_qual_decoder;
typedef struct cl_id_decoder cl_id_decoder;
/* CDNACoder::Init(false, ...) + CReferenceReads + CRefReadsAccepter: max_alt_refs / level (1-3; 9 = the models of the stored reference genome) / sparse range + exponent come from the
 * archive's `meta` stream; accept_all = ReferenceReadsMode::All; start_read_id = n_pseudo for single-domain archives. */
cl_status cl_dna_decoder_create(uint32_t max_alt_refs, int32_t level, uint32_t start_read_id, uint32_t n_pseudo,
                                int32_t accept_all, uint32_t sparse_range, double sparse_exponent, cl_dna_decoder** out);
void cl_dna_decoder_free(cl_dna_decoder* d);
const char* cl_dna_decoder_error(const cl_dna_decoder* d);
/* a reference-genome pseudo read (codes 0..3), in order, before the first part (decompression_common.cpp:300-305) */
cl_status cl_dna_decoder_add_ref(cl_dna_decoder* d, const uint8_t* h_codes, uint32_t len);
/* Archives written by several GPUs hold one model domain per rank: fresh adaptive models from here on; the reference reads, the
 * read counter and the acceptor's random stream continue. */
cl_status cl_dna_decoder_new_domain(cl_dna_decoder* d);
/* One `dna` part of n_reads reads (the part's archive metadata) -> bases back to back: codes 0..3, 4 = N, at levels 2 and 3 with
 * the class flags 0x80 (anchor) / 0x40 (match) the quality decoder reads (basic_coder.h:34-35); h_off[n_reads+1].  If cap is too
 * small: CL_E_CAPACITY with *n_out = bytes needed; the decoded part stays inside the decoder and the same call with a buffer of
 * that size fetches it (nothing is decoded twice).  cl_id_decode_part behaves the same way. */
cl_status cl_dna_decode_part(cl_dna_decoder* d, const uint8_t* h_in, uint64_t n_in, uint32_t n_reads,
                             uint8_t* h_bases, uint64_t cap, uint64_t* h_off, uint64_t* n_out);
/* CQualityCoder::Init(false, ...): params as for the encoder; rev[] = the representatives stored in `meta` (-D). */
cl_status cl_qual_decoder_create(const cl_qual_params* params, cl_qual_decoder** out);
void cl_qual_decoder_free(cl_qual_decoder* q);
cl_status cl_qual_decoder_new_domain(cl_qual_decoder* q);
/* One `qual` part: h_bases / h_off are the output of cl_dna_decode_part for the same part; h_quals receives ASCII qualities at
 * the same offsets. */
cl_status cl_qual_decode_part(cl_qual_decoder* q, const uint8_t* h_in, uint64_t n_in, const uint8_t* h_bases, const uint64_t* h_off,
                              uint32_t n_reads, uint8_t* h_quals);
/* The qual digest of what the decoder decodes (off by default: one flag test per read).  on: from the next read on, read by read,
 * the symbols as they leave the models — before the -D representatives and the error diffusion turn them into quality values, which
 * the digest does not cover — and the average bytes are digested, the next read being read first_read of the input; the totals start
 * from zero.  Mode none decodes nothing and digests nothing.  cl_qual_decoder_digest: the totals so far. */
cl_status cl_qual_decoder_set_digest(cl_qual_decoder* q, int on, uint64_t first_read);
cl_status cl_qual_decoder_digest(const cl_qual_decoder* q, cl_digest* out);
/* The `qual` parts of whole model domains decoded ON THE DEVICE, one lane per domain (k_qual_decode): CEntrDecomprQuals
 * (entr_qual.h:136-260) over CQualityCoder::Decode (quality_coder.cpp:605-657, quality_coder_impl.cpp:506-559,800-849) and
 * CRangeDecoder (sub_rc.h:216-392).  params: as for cl_qual_decoder_create (the -T thresholds may be left out, n_fwd = 0: a decoder
 * never maps a quality to its bin).  reads: the arena of the decoded bases of the parts' reads (cl_reads_pack; the contexts use
 * neighbouring bases, N as A); part p holds the reads [h_part_bounds[p], h_part_bounds[p + 1]); d_flags: their classes in the form of
 * cl_es_flags at the offsets d_qual_off (levels 2 and 3; null at level 1); d_in (n_in bytes): the part payloads back to back,
 * h_part_sizes[n_parts]; domain d = the parts [h_domain_first_part[d], h_domain_first_part[d + 1]) (the first entry 0, ascending; the
 * last domain ends with the parts).  Output: ASCII qualities at d_qual_off (n_reads + 1 offsets that hold the arena's read lengths, all
 * inside quals_cap) — byte for byte what cl_qual_decode_part gives for the same parts with cl_qual_decoder_new_domain at every domain
 * start — and, with d_symbols (symbols_cap bytes; null: not wanted), the symbols as they leave the models, read r at
 * r * navg + d_qual_off[r] (avg: r * 2; navg = the average bytes of the mode): its average bytes, then one byte per base, the order
 * cl_digest_quals defines (digest them with cl_digest_bytes_host, kind 2).  Every domain has model tables of its own in device memory
 * (n_ctx x (n_sym + 1) + 896 x 257 words: 0.7 MB for 4-avg, 13 MB for org at level 1, 102 MB at level 3): a launch decodes as many
 * domains as fit COLORD_HIP_QDEC_BUDGET_MB (default 4096) and at most max_domains_per_launch (0: no limit of its own), further
 * launches take the rest.  A part that does not decode (a symbol outside its model's interval) or does not end at its size:
 * CL_E_MISMATCH, the text naming the first such domain and its part; that domain stops there, every other domain is decoded
 * completely.  No input makes the kernel read or write out of range: bytes past a part's size read as 0, a part decodes exactly the
 * symbols its reads' lengths ask for. */
cl_status cl_qual_decode_domains(cl_ctx* ctx, const cl_qual_params* params, const cl_reads* reads, const uint8_t* d_flags,
                                 const uint8_t* d_in, uint64_t n_in, const uint32_t* h_part_bounds, const uint64_t* h_part_sizes, uint32_t n_parts,
                                 const uint32_t* h_domain_first_part, uint32_t n_domains, uint32_t max_domains_per_launch,
                                 uint8_t* d_quals, const uint64_t* d_qual_off, uint64_t quals_cap, uint8_t* d_symbols, uint64_t symbols_cap);
cl_status cl_id_decoder_create(int32_t header_mode, cl_id_decoder** out);
void cl_id_decoder_free(cl_id_decoder* c);
/* One `header` part of n ids -> the ids back to back (without '@' / '>'), h_off[n+1], h_plus[n] (1 = the '+' line repeats the id). */
cl_status cl_id_decode_part(cl_id_decoder* c, const uint8_t* h_in, uint64_t n_in, uint32_t n, uint8_t* h_ids, uint64_t cap,
                            uint64_t* h_off, uint8_t* h_plus, uint64_t* n_out);

/* ---- a7: CReferenceReads (reference_reads.h:27-259) ---------------------------------------------- */
/* Byte image of one stored reference read (4 bases/byte MSB first + trailing count byte) produced from
 * the arena; h_out needs (len+3)/4+1 bytes.  Used by the parity tests and by the host archive code. */
cl_status cl_reads_compact(cl_ctx* ctx, const cl_reads* reads, uint32_t read, uint8_t* h_out, uint64_t cap, uint64_t* n_out);

/* ---- utilities (device primitives exposed for tests/bench) -------------------------------------- */
cl_status cl_sort_u64(cl_ctx* ctx, uint64_t* d_keys, uint64_t n, uint32_t begin_bit, uint32_t end_bit);
cl_status cl_sort_u64_u32(cl_ctx* ctx, uint64_t* d_keys, uint32_t* d_vals, uint64_t n, uint32_t begin_bit, uint32_t end_bit);
/* Stable LSD radix sort on the key bits [begin_bit, end_bit) — whole keys travel, bits outside the range never order anything;
 * end_bit beyond the key's width is CL_E_INVALID.  d_vals may be null in cl_sort_u32_u32 (keys only). */
cl_status cl_sort_u32(cl_ctx* ctx, uint32_t* d_keys, uint64_t n, uint32_t begin_bit, uint32_t end_bit);
cl_status cl_sort_u32_u32(cl_ctx* ctx, uint32_t* d_keys, uint32_t* d_vals, uint64_t n, uint32_t begin_bit, uint32_t end_bit);
/* The same sorts in the form the coders call: on pool buffers of exactly n elements that may come back exchanged with the sort's
 * temporaries instead of being copied into.  The input arrays are left as they are; the result goes to d_keys_out / d_vals_out. */
cl_status cl_sort_swap_u32_u32(cl_ctx* ctx, const uint32_t* d_keys_in, const uint32_t* d_vals_in, uint64_t n, uint32_t begin_bit, uint32_t end_bit,
                               uint32_t* d_keys_out, uint32_t* d_vals_out);
cl_status cl_sort_swap_u64_u32(cl_ctx* ctx, const uint64_t* d_keys_in, const uint32_t* d_vals_in, uint64_t n, uint32_t begin_bit, uint32_t end_bit,
                               uint64_t* d_keys_out, uint32_t* d_vals_out);
/* In-place exclusive prefix sums of n uint32; *h_total (optional) = the sum.  With h_total a sum of 2^32 or more is refused
 * (CL_E_UNSUPPORTED; the array then holds meaningless prefixes); without it nothing is checked. */
cl_status cl_scan_u32(cl_ctx* ctx, uint32_t* d_data, uint64_t n, uint64_t* h_total);
/* d_out[0 .. n] = exclusive prefix sums of d_in[0 .. n) in 64 bits, d_out[n] = *h_total (optional) = the sum.  With h_total a sum of
 * 2^52 - 1 or more is refused (CL_E_UNSUPPORTED). */
cl_status cl_scan_u32_u64(cl_ctx* ctx, const uint32_t* d_in, uint64_t* d_out, uint64_t n, uint64_t* h_total);
/* Starts of the runs of equal `key >> shift` in sorted keys: d_seg[0 .. r) = first positions, d_seg[r] = n, *h_n_runs = r.  seg_cap
 * (elements of d_seg) MUST exceed r — the caller bounds it by n and by the distinct values of key >> shift; the kernel has written by
 * the time CL_E_CAPACITY is returned.  shift at or beyond the key's width is CL_E_INVALID, n >= 2^32 CL_E_UNSUPPORTED. */
cl_status cl_run_starts_u32(cl_ctx* ctx, const uint32_t* d_keys, uint64_t n, uint32_t shift, uint32_t* d_seg, uint64_t seg_cap, uint64_t* h_n_runs);
cl_status cl_run_starts_u64(cl_ctx* ctx, const uint64_t* d_keys, uint64_t n, uint32_t shift, uint32_t* d_seg, uint64_t seg_cap, uint64_t* h_n_runs);

#ifdef __cplusplus
}
#endif
#endif
