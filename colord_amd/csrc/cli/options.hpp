// options.hpp — the options of `colord_hip compress-*`: the reference's (src/colord/arg_parse.cpp:455-640 options and their checks, :89-408
// presets, :32-84,410-450 quality thresholds) and this build's own.  Both drivers (compress.cpp, compress_multi.cpp) start from parse_options().
#pragma once
#include "archive.hpp"
#include <cctype>
#include <cstdlib>

struct Preset { int level; uint32_t ci, cs, f, c, max_rec, min_part_alt; int qual_mode; int sparse; double g; };
// arg_parse.cpp:89-408 — [source][priority]: ratio, balanced, memory (memory is the default priority)
inline const Preset PRESETS[3][3] = {
	{ { 3, 2, 120, 8, 10, 6, 48, 2, 0, 1 }, { 2, 3, 100, 9, 8, 5, 48, 2, 1, 2 }, { 1, 4, 80, 12, 5, 3, 64, 2, 1, 1 } },          // ONT, 4-avg qualities
	{ { 3, 2, 120, 8, 10, 6, 48, 8, 0, 1 }, { 2, 3, 100, 9, 8, 5, 48, 8, 1, 2 }, { 1, 4, 80, 12, 5, 3, 64, 8, 1, 1 } },          // PBRaw, qualities dropped
	{ { 3, 2, 150, 20, 12, 6, 48, 1, 0, 1 }, { 2, 3, 120, 30, 10, 5, 48, 1, 1, 6 }, { 2, 3, 100, 40, 8, 5, 48, 1, 1, 3 } },       // PBHiFi, 5-avg qualities
};
// default -T / -D values of the quality modes (arg_parse.cpp:32-84,410-450): mode -> forward thresholds, decoder representatives
struct QDef { std::vector<uint32_t> fwd, rev; };
inline QDef qual_defaults(int mode)
{
	static const QDef defs[9] = { {}, { { 7, 14, 26, 93 }, {} }, { { 7, 14, 26 }, {} }, { { 7 }, {} }, { { 7, 14, 26, 93 }, { 3, 10, 18, 35, 93 } }, { { 7, 14, 26 }, { 3, 10, 18, 35 } }, { { 7 }, { 1, 13 } }, {}, { {}, { 0 } } };
	return defs[mode];
}
inline const char* const QUAL_MODE_NAMES[9] = { "org", "5-avg", "4-avg", "2-avg", "5-fix", "4-fix", "2-fix", "avg", "none" };      // QualityComprMode (params.h:33-43)
inline int qual_mode_of(const std::string& s) { for (int i = 0; i < 9; ++i) if (s == QUAL_MODE_NAMES[i]) return i; return -1; }
inline std::vector<uint32_t> list_u32(const std::string& s) { std::vector<uint32_t> v; size_t p = 0; while (p < s.size()) { size_t e = s.find_first_of(", ", p); if (e == std::string::npos) e = s.size(); if (e > p) v.push_back((uint32_t)strtoul(s.substr(p, e - p).c_str(), nullptr, 10)); p = e + 1; } return v; }

struct Options {
	int source = 0, prio = 2, gpu = 0; bool verbose = false;
	uint32_t k = 0, a = 0; std::string in, out, genome; bool store_genome = false;
	long ci = -1, cs = -1, f = -1, c = -1, max_rec = -1, min_to_alt = -1, min_anchors = 1;
	double cost_mult = 1.0, frac_min = 0.5, frac_always = 0.9, max_matches_mult = 10.0, g = -1, exponent = 1.0;
	int qual_mode = -1, header_mode = 0, ref_mode = -1;
	std::vector<uint32_t> T, D; bool has_T = false, has_D = false;
	double chunk_bases = 1.0e9; bool chunk_bases_set = false;
	uint64_t part_symbols = 2u << 21;               // --part-symbols: the coder parts close once their reads (+ 1 guard each) reach this; default = the reader packs (defs.h:45)
	int parse_threads = 0;                          // --parse-threads (0: as many as the host offers, at most 32)
	bool stream_input = false;                      // --stream-input: the input is read three times (k-mers, reference reads, coding) and only a window of chunks is resident in HBM
	int domains = 1;                                // --domains K: K INDEPENDENT model domains on one GPU (own k-mer set, references, index, models each): decoded side by side
	bool verify_scripts = false;                    // --verify-scripts: cl_ctx_set_verify on every compressor's context
	bool verify_streams = false;                    // --verify-streams: cl_ctx_set_verify_streams on every compressor's context
	bool digest = false;                            // --digest: content digests of the input (cl_ctx_set_digest; ids on the host) in a `hipdigest` stream
	bool digest_values = false;                     // --digest-values: --digest and the qual-values digest (cl_ctx_set_digest_values); `hipdigest` version 2
	bool report = false;                            // --report: the content report of the input (cl_ctx_set_report) in a `hipreport` stream
	bool edit_profile = false;                      // --edit-profile: the edit-operation profile of the tuple streams (cl_ctx_set_edit_profile) in a `hipedits` stream
	bool kmer_spectrum = false;                     // --kmer-spectrum: the count spectrum of the k-mers pass 1 counted (cl_ctx_set_kmer_spectrum) in a `hipkmers` stream
	bool sketch = false; long sketch_size = -1, sketch_min_count = -1;   // --sketch [--sketch-size N] [--sketch-min-count M]: the MinHash sketch of the k-mers pass 1 counted at least M times (cl_ctx_set_kmer_sketch) in a `hipsketch` stream; defaults 10 000 and 2
	bool mappings = false;                          // --mappings (with -G): the read-to-genome alignments the edit scripts hold (cl_ctx_set_mappings) in a `hipmappings` stream
	bool cigars = false;                            // --cigars (with --mappings): the base-level CIGAR of every mapping record (cl_ctx_set_cigars) in a `hipcigars` stream
	bool cigars_coded = false;                      // --cigars-coded (with --cigars): the operations are coded on the device (cl_ctx_set_cigars_coded); `hipcigars` version 2
	bool pileup = false; long pileup_min_depth = -1, pileup_min_alt = -1; double pileup_min_frac = -1;   // --pileup (with -G) [--pileup-min-depth N] [--pileup-min-alt N] [--pileup-min-frac F]: the per-position base counts of the reads on the genome's pieces (cl_ctx_set_pileup); their sites in a `hippileup` stream; defaults 4, 3 and 0.25
	bool overlaps = false;                          // --overlaps: the read-to-read overlaps the edit scripts hold (cl_ctx_set_overlaps) in a `hipoverlaps` stream
	uint64_t qual_domain_symbols = 0;               // --qual-domain-symbols N: the quality models start afresh about every N symbols (cl_compressor_set_qual_domain_symbols; stream `hipqdomains`)
	int gpus = 1; std::vector<int> gpu_list; std::string transport = "rccl";   // --gpus N [--gpu-list a,b,..] [--transport rccl|host]: reads sharded over N GPUs (run_compress_multi)
	Preset P{}; QDef qd;                            // resolved by parse_options: the preset of source and priority with the options laid over it, the quality thresholds / representatives
	int argc = 0; char** argv = nullptr;            // the command line as given (`info` stream)
};

inline void usage()
{
	fprintf(stderr,
		"usage: colord_hip compress-ont|compress-pbhifi|compress-pbraw [options] input.fastq|fasta[.gz] output.colord\n"
		"       colord_hip decompress [--ignore-digest] [--gpu N] archive.colord output.fastq\n       colord_hip check [--gpu N] archive.colord\n       colord_hip info [--report [--json]] [--edit-profile [--json]] [--kmer-spectrum [--json]] archive.colord\n       colord_hip info --overlaps [--min-block N] [--names] archive.colord\n       colord_hip info --mappings [--min-block N] [--names] | --mappings --coverage W | --mappings --summary [--json] archive.colord\n       colord_hip info --mappings --cigar | --mappings --sam [--min-block N] [--names] archive.colord\n       colord_hip info --pileup [--min-alt N] [--min-frac F] [--vcf] | --pileup --summary [--json] archive.colord\n       colord_hip info --sketch [--json] archive.colord\n       colord_hip dist [--json] A.colord B.colord [C.colord ...]\n"
		"options (as the reference, arg_parse.cpp:455-640):\n"
		"  -p,--priority ratio|balanced|memory   -k,--kmer-len K with -a,--anchor-len A (both or none)\n"
		"  -q,--qual org|none|avg|2-fix|4-fix|5-fix|2-avg|4-avg|5-avg   -T,--qual-thresholds a,b,..   -D,--qual-values a,b,..\n"
		"  -i,--identifier org|main|none   -c,--max-candidates N   -L,--Lowest-count N   -H,--Highest-count N   -f,--filter-modulo N\n"
		"  -e,--edit-script-mult X   -r,--max-recurence-level N   --min-to-alt N   --min-mmer-frac X   --min-mmer-force-enc X\n"
		"  --max-matches-mult X   --min-anchors N   -R,--Ref-reads-mode all|sparse   -g,--sparse-range X   -x,--sparse-exponent X\n"
		"  -t,--threads N (accepted; the data path runs on the GPU)   -v,--verbose   --gpu N   --chunk-bases X\n"
		"  --part-symbols N   coder parts of N symbols instead of the reference's 4194304 (defs.h:45): same FASTQ back from either\n"
		"                     decompressor, 8 more bytes per part, far shorter interval-coder chains (65536: +0.04 %% size, 1.4x the speed)\n"
		"  --parse-threads N  threads that index a plain FASTQ (default: the host's, at most 32)\n"
		"  --stream-input     bounded device memory: the input is read three times (k-mers, reference reads, coding) and only a window of\n"
		"                     four chunks is resident at a time instead of the whole input (same archive)\n"
		"  --verify-scripts   every read is rebuilt on the device from its edit script and the reference reads and compared with the input; the entropy-coded bytes are not decoded\n"
		"                     (a read that differs: message, no archive, non-zero exit)\n"
		"  --verify-streams   each coded part of the dna and qual streams is decoded on the device with the decoder's interval arithmetic: every symbol must fall in the interval\n"
		"                     its model gave it and the part must end at its size; the models themselves are not replayed (edit scripts -> sort keys -> triples is not covered)\n"
		"                     (a part that does not decode: message, no archive, non-zero exit)\n"
		"  --digest           content digests of the input — bases and quality symbols digested on the device before any kernel of the compressor touches them, ids on the host —\n"
		"                     are stored in the archive (stream `hipdigest`, 80 bytes; the reference's decompressor ignores it).  `colord_hip decompress` recomputes them from what it\n"
		"                     decodes: a difference is a message naming the stream, no output file and exit 1 (--ignore-digest decodes regardless); `colord_hip check` decodes without\n"
		"                     writing and prints them.  Same digest with any --part-symbols, --stream-input, --domains, --gpus.  Covered: input -> ... -> decoded symbols; the quality\n"
		"                     VALUES made from the symbols (-D values, error diffusion of *-avg) are covered by --digest-values.  Cost: one pass over 1.4 bytes per base per chunk (not measured on a GPU yet)\n"
		"  --digest-values    --digest, and a fourth digest, qual-values: the quality VALUES every record must decode to (org: the value; *-fix: the -D value of its bin; *-avg, avg:\n"
		"                     the error diffusion of the bin's average, as integers), made on the device from the input qualities alone and stored with the other three (`hipdigest`\n"
		"                     version 2, 104 bytes).  `colord_hip decompress` / `check` digest the quality bytes as they are handed to the writer, whichever decoder made them (host, or\n"
		"                     --gpu): the hole --digest leaves between the decoded symbols and the quality line is closed.  With -q none or FASTA input there are no values: as --digest.\n"
		"                     Cost: one more pass over the quality bytes per chunk, two in the *-avg modes (not measured on a GPU yet)\n"
		"  --report           a content report of the input, counted on the device before any kernel of the compressor touches it, is stored in the archive (stream `hipreport`; the\n"
		"                     reference's decompressor ignores it): reads, bases, base composition (A C G T N), read lengths (min, max, histogram by bit length, N50, N90) and, with a\n"
		"                     coded quality stream, the exact joint distribution of INPUT quality against the quality VALUE the archive decodes to (the quantity of --digest-values), and\n"
		"                     the reads' mean qualities — the arithmetic mean of the Phred values per read, NOT the error-probability mean other tools print.  `colord_hip info --report\n"
		"                     [--json]` prints it without decoding anything, with the share of bases unchanged, MAE, RMSE and max |delta| of the quality mode.  `colord_hip decompress` /\n"
		"                     `check` recompute the output side (reads, bases, composition, lengths, N50, N90, the stored values' distribution) from what they decode: a difference names\n"
		"                     the first differing field with both numbers, no output file and exit 1 (--ignore-digest decodes regardless).  The INPUT side cannot be recomputed from a lossy\n"
		"                     archive and is not checked.  Same report with any --part-symbols, --stream-input, -G [-s], --domains, --gpus: all of them read the input through one reader in\n"
		"                     one process, which has every read length for N50 / N90.  A *-fix mode needs -D values <= 95.  With -q none or FASTA input there is no quality part.\n"
		"                     Cost: one pass over 0.375 bytes per base and one over the quality bytes per chunk, two in the *-avg modes (not measured on a GPU yet)\n"
		"  --edit-profile     what the compressor did with the bases, counted on the device from every read's edit script right after it was made, is stored in the archive (stream `hipedits`,\n"
		"                     2504 bytes; the reference's decompressor ignores it): reads coded plain / with an edit script, tuples by type, anchor and skip lengths, the substitution matrix,\n"
		"                     inserted, deleted and matched base composition, insertion and deletion run lengths, identity per read, alternative references per read.  `colord_hip info\n"
		"                     --edit-profile [--json]` prints it without decoding anything, with the rates per aligned base, transitions : transversions and the identity median.  THIS IS THE\n"
		"                     DIVERGENCE BETWEEN A READ AND THE REFERENCE READS IT WAS CODED AGAINST, and both carry errors: it is not a per-read error rate, except against the pseudo reads\n"
		"                     of -G; and it covers only what the encoder aligned (plain reads and skipped stretches say nothing).  `decompress` / `check` do not recompute it.  Works with\n"
		"                     --stream-input, -G [-s], --part-symbols, --chunk-bases; with --gpus / --domains every domain has its own reference reads and the parts are added.\n"
		"                     Cost: one pass over the tuple bytes per chunk; measured on an MI355X: 2.17 ms of kernel time for a 5-Mbase ONT chunk (1 025 reads, 3.8 MB of tuples), next to 2.31 ms of\n"
		"                     the --verify-scripts pass and 753 ms of all kernels of that chunk (DESIGN.md 9)\n"
		"  --kmer-spectrum    the count spectrum of the sampled k-mers — how many distinct k-mers occur once, twice, and so on — taken on the device from the sorted keys of pass 1, BEFORE the cut\n"
		"                     at -L and the saturation at -H, is stored in the archive (stream `hipkmers`, 33 352 bytes; the reference's decompressor ignores it): exact bins for the counts\n"
		"                     1..4095, bins by bit length with their mass above.  `colord_hip info --kmer-spectrum [--json]` prints it without decoding anything, with what -L dropped and -H\n"
		"                     flattened, the kept k-mers (the `meta` stream's numbers) and — for one k-mer set of reads alone — the valley, the coverage peak and a genome-size estimate.  THE\n"
		"                     K-MERS ARE THE 1-IN-f HASH SAMPLE (-f), the peak is the depth of error-free k-mers, not of bases, and the size is an estimate.  Works with --stream-input, --gpus N\n"
		"                     (the ranks own disjoint key ranges of one set: sets = 1), --domains K (K sets added, no estimate) and -G [-s] (the genome's k-mers are counted too: flag bit 0,\n"
		"                     no estimate).  `decompress` / `check` do not recompute it.  Cost: one pass over 4 bytes per distinct sampled k-mer;\n"
		"                     measured on an MI355X, 400 Mbases of synthetic ONT reads (33.3 M sampled k-mers, 27.6 M distinct): k_run_spectrum 0.077 ms of kernel time next to 2.61 ms of all kernels of\n"
		"                     the same count, 0.10 ms of wall time on 2.90 ms; at 5 Gbases in the benchmark about 1 ms in a pass of 1.9 s, inside the run-to-run spread (DESIGN.md 9)\n"
		"  --sketch [--sketch-size N] [--sketch-min-count M]   a bottom-N MinHash sketch of the sampled k-mers that occur at least M times (defaults 10 000 and 2; N up to 1 048 576) is made\n"
		"                     on the device from the sorted keys of pass 1 and stored in the archive (stream `hipsketch`, 48 + 16 bytes per entry, 160 KB by default; the reference's\n"
		"                     decompressor ignores it): the N smallest values of a 64-bit hash of the k-mers, each with the k-mer's count.  `colord_hip info --sketch [--json]` prints it,\n"
		"                     `colord_hip dist [--json] A.colord B.colord [C.colord ...]` compares A with each of the others — Jaccard index, containment both ways and the distance\n"
		"                     -ln(2j / (1 + j)) / k — from the sketches alone (tab-separated: A, B, distance, jaccard, shared, compared, containment of A, of B): no GPU, nothing decoded.  THE K-MERS ARE THE 1-IN-f HASH SAMPLE (-f) of reads with errors, cut at M (ONT\n"
		"                     singletons are nearly all errors): sketches compare ONLY AT EQUAL k AND f, and the distance is not comparable with Mash distances of assembled genomes.\n"
		"                     Works with --stream-input, --gpus N (the ranks own disjoint key ranges of one set: sets = 1, the same bytes), --domains K (K sets merged: M applies per set,\n"
		"                     `qualifying` is a sum over the sets) and -G [-s] (the genome's k-mers are counted too: flag bit 0).  `decompress` / `check` ignore the stream.\n"
		"                     Cost: two passes over 4 bytes per distinct sampled k-mer, 8 bytes per k-mer that occurs M times, and a sort of a few thousand pairs;\n"
		"                     measured on an MI355X, 400 Mbases of synthetic ONT reads (27.6 M distinct sampled k-mers, 2.1 M of them counted twice or more): k_sketch_bins 0.146 ms, k_sketch_take\n"
		"                     0.149 ms and 0.21 ms of sort kernels next to 2.68 ms of all kernels of the same count, 0.81 ms of wall time on 3.01 ms; from file to archive inside the spread of\n"
		"                     three runs (DESIGN.md 4l, 9)\n"
		"  --overlaps         the read-to-read overlaps that the edit scripts hold are stored in the archive (stream `hipoverlaps`, 48 bytes per record; the reference's decompressor ignores it):\n"
		"                     one record per stretch of a read's edit script on ONE reference read that holds an aligned column — where on the read, where on the reference read in its\n"
		"                     forward coordinates, strand, matches, substitutions, anchor bases — made on the device right behind the edit scripts.  `colord_hip info --overlaps\n"
		"                     [--min-block N] [--names] archive` prints them as PAF without decoding `dna` or `qual` (tags mm:i: substitutions, an:i: anchor bases, tp:A:P the main reference,\n"
		"                     tp:A:S an alternative; names are input indices unless --names decodes the `header` stream).  THIS IS A READ AGAINST EARLIER READS, WHICH CARRY ERRORS OF\n"
		"                     THEIR OWN, AND IT LISTS OVERLAPS WITH REFERENCE READS ONLY: about a tenth of the reads with the sparse acceptor (-R sparse), all of them with -R all.\n"
		"                     `decompress` / `check` ignore the stream.  Works with --stream-input, --part-symbols, --chunk-bases.  Not with --gpus > 1, --domains > 1 or -G.\n"
		"                     Cost: one pass over the tuple bytes per chunk to count and one to fill; measured on an MI355X, 1 Gbase of synthetic ONT reads (64 156 reads): 12.2 + 12.9 ms of kernel\n"
		"                     time next to 23.5 ms of --edit-profile and 962 ms of all kernels; 1.77 s from file to archive against 1.69 s without the option, inside the spread of three runs;\n"
		"                     88 989 records, 4.3 MB, 1.1 percent of the archive (DESIGN.md 9)\n"
		"  --mappings         with -G: the read-to-genome alignments that the edit scripts hold are stored in the archive (stream `hipmappings`, 48 bytes per record and the genome's sequence\n"
		"                     names and lengths; the reference's decompressor ignores it): the genome's overlapping pieces are the first reference reads, and every stretch of a read's edit\n"
		"                     script on ONE piece that holds an aligned column is one record, lifted on the device to the coordinates of the sequence the piece was cut from.\n"
		"                     `colord_hip info --mappings [--min-block N] [--names] archive` prints them as PAF with the FASTA's sequence names, `info --mappings --coverage W` a bedGraph\n"
		"                     track of the mean depth in windows of W bases, `info --mappings --summary [--json]` what they add up to; none decodes `dna` or `qual` or needs a GPU.\n"
		"                     WHAT IT IS NOT: A READ CODED AGAINST EARLIER READS INSTEAD OF GENOME PIECES YIELDS NO RECORD, AND A READ THAT SPANS A PIECE BOUNDARY YIELDS ONE RECORD PER\n"
		"                     PIECE; THESE ARE NOT STITCHED.  `decompress` / `check` ignore the stream.  Works with --stream-input, --part-symbols, --chunk-bases and every other view.\n"
		"                     Not without -G, not with --gpus > 1, --domains > 1 or --overlaps.  Cost: the walk of --overlaps and 48 bytes read and written per record (DESIGN.md 4m, 9)\n"
		"  --cigars           with --mappings: the base-level CIGAR of every mapping record, made on the device by a third walk of the tuple bytes, stored in the archive (stream `hipcigars`:\n"
		"                     a count per record and four bytes per operation, len << 4 | op with BAM's codes for I, D, = and X; the reference's decompressor ignores it).  From the record's\n"
		"                     first aligned column to its last; neighbouring equal operations are merged.  `colord_hip info --mappings --cigar archive` prints the PAF of --mappings with\n"
		"                     cg:Z: appended, `info --mappings --sam` SAM (a line per record; the second and later records of a read are supplementary, unaligned read ends are hard clips,\n"
		"                     no sequence); neither decodes `dna` or `qual` or needs a GPU.  NOT COMPRESSED: THE STREAM IS LARGER THAN THE `dna` STREAM — measured on an\n"
		"                     MI355X, 300 Mbases of synthetic ONT reads on a 15-Mbase genome: 39.5 M operations, 158 MB, 0.53 bytes per input base, 7.5 times the `dna` stream and 63 percent\n"
		"                     of the archive; 2.55 s from file to archive against 2.16 s with --mappings alone.  It is opt-in; --cigars-coded stores it coded.\n"
		"                     = and X are not collapsed to M.  `decompress` / `check` ignore the stream.  Not without --mappings, and so not with\n"
		"                     --gpus > 1, --domains > 1 or --overlaps (DESIGN.md 4o, 9)\n"
		"  --cigars-coded     with --cigars: the operations are coded ON THE DEVICE before they leave it (stream `hipcigars` version 2): an op symbol in the context of the op before and a\n"
		"                     length symbol in the context of its op (lengths above 255 escape to a raw u32), a static table per segment of 2^20 operations, the interval coder of the\n"
		"                     `dna` and `qual` streams over parts of 4096 operations.  `info --mappings --cigar | --sam` print the same text from either version; `colord_hip info` adds the coded\n"
		"                     bytes, bytes per operation and the escapes.  On the run above: 18.3 MB instead of 158 MB (0.46 bytes per operation, 0.87 times the `dna` stream), 3.05 s against 2.53 s.  Without it every byte is as before.  Not made for HiFi-like inputs, whose = runs are mostly escapes (DESIGN.md 4p)\n"
		"  --pileup           with -G: per-position base counts of the reads on the genome, made on the device from the edit scripts: for every genome position the read columns that match, that say\n"
		"                     A, C, G or T instead (in the genome's forward orientation), that delete it, and the insertion RUNS left of which it lies (a run counts once: unaligned read ends are\n"
		"                     coded as long runs).  THE FULL TABLE IS NOT STORED, it is the size of the genome: the archive gets its totals and its SITES (stream `hippileup`, 48 bytes per site and\n"
		"                     the genome's sequence names and lengths; the reference's decompressor ignores it) — positions of depth >= --pileup-min-depth N (4) whose strongest alternative has\n"
		"                     >= --pileup-min-alt N (3) columns and >= --pileup-min-frac F (0.25) of the depth.  The defaults are interface defaults, chosen so that isolated read errors do not\n"
		"                     qualify at ONT error rates; THEY ARE NOT TUNED AGAINST ANYTHING.  `colord_hip info --pileup [--min-alt N] [--min-frac F] archive` prints the sites as a table (name, 1-based\n"
		"                     position, ref, depth, A, C, G, T, del, ins, kind; the options can only tighten what was stored), `info --pileup --vcf` the base sites as a minimal VCF 4.2,\n"
		"                     `info --pileup --summary [--json]` totals, mean depth, rates and sites per kind; none decodes `dna` or `qual` or needs a GPU.  READS CODED AGAINST EARLIER READS INSTEAD OF\n"
		"                     GENOME PIECES COUNT NOTHING; there are no per-strand counts.  Independent of --mappings (both may be given).  Not without -G, not with --gpus > 1, --domains > 1 or\n"
		"                     --overlaps.  Cost: one more walk of the tuple bytes per chunk and 36 bytes of device memory per genome position (DESIGN.md 4n, 9)\n"
		"  --qual-domain-symbols N   model domains of the QUALITY stream alone: its adaptive models start afresh at the first part boundary at which a domain holds N coded\n"
		"                     symbols, and the starts are recorded (stream `hipqdomains`).  `colord_hip decompress --gpu N` / `check --gpu N` then decode the domains side by\n"
		"                     side on the device, one lane each; without --gpu they decode on the host as one chain that starts afresh at every domain.  The k-mer set, the\n"
		"                     reference reads and the `dna`, `header` and `hipdigest` streams are untouched.  The reference's decompressor CANNOT read such an archive: it\n"
		"                     ignores the stream and carries its models on.  Costs `qual` bytes per domain (the models relearn; NOT measured yet — no size table exists, DESIGN.md 9 has the protocol).  Not with --gpus > 1,\n"
		"                     --domains > 1 or -q none\n"
		"  --domains K        K independent model domains (equal shares of the reads, each compressed on its own): `colord_hip decompress`\n"
		"                     decodes them side by side; costs archive size (own k-mer statistics and reference reads per domain)\n"
		"  --gpus N [--gpu-list a,b,..] [--transport rccl|host]   reads sharded over N GPUs, one host thread and one model domain per GPU;\n"
		"                     the k-mer set, reference reads and index are replicated through RCCL (or host staging: several ranks per GPU)\n");
}

// the command line of a compress-* mode with every check of the reference (arg_parse.cpp:604-625) and of this build; -h ends the process
inline Options parse_options(int argc, char** argv)
{
	Options O; O.argc = argc; O.argv = argv;
	const std::string mode = argv[1];
	O.source = mode == "compress-ont" ? 0 : mode == "compress-pbraw" ? 1 : mode == "compress-pbhifi" ? 2 : -1;
	if (O.source < 0) { usage(); die("unknown mode " + mode); }
	std::vector<std::string> pos;
	auto need = [&](int& i) -> std::string { if (i + 1 >= argc) die(std::string("option ") + argv[i] + " needs a value"); return argv[++i]; };
	// (-T 5 12 30: values separated by spaces are taken as long as two positional arguments remain)
	auto more_values = [&](int& i, std::vector<uint32_t>& v) { while (i + 1 < argc && isdigit((unsigned char)argv[i + 1][0]) && pos.size() + (size_t)(argc - i - 1) > 2) v.push_back((uint32_t)atoi(argv[++i])); };
	for (int i = 2; i < argc; ++i)
	{
		const std::string a = argv[i];
		if (a == "-p" || a == "--priority") { const std::string v = need(i); O.prio = v == "ratio" ? 0 : v == "balanced" ? 1 : v == "memory" ? 2 : -1; if (O.prio < 0) die("unknown priority " + v); }
		else if (a == "-k" || a == "--kmer-len") { O.k = (uint32_t)atoi(need(i).c_str()); if (O.k < 15 || O.k > 28) die("-k,--kmer-len must be in [15, 28]"); }
		else if (a == "-a" || a == "--anchor-len") O.a = (uint32_t)atoi(need(i).c_str());
		else if (a == "-q" || a == "--qual") { const std::string v = need(i); O.qual_mode = qual_mode_of(v); if (O.qual_mode < 0) die("unknown quality mode " + v); }
		else if (a == "-T" || a == "--qual-thresholds") { O.T = list_u32(need(i)); O.has_T = true; more_values(i, O.T); }
		else if (a == "-D" || a == "--qual-values") { O.D = list_u32(need(i)); O.has_D = true; more_values(i, O.D); }
		else if (a == "-i" || a == "--identifier") { const std::string v = need(i); O.header_mode = v == "org" ? 0 : v == "main" ? 1 : v == "none" ? 2 : -1; if (O.header_mode < 0) die("unknown header mode " + v); }
		else if (a == "-c" || a == "--max-candidates") { O.c = atol(need(i).c_str()); if (O.c < 1) die("-c must be positive"); }
		else if (a == "-L" || a == "--Lowest-count") O.ci = atol(need(i).c_str());
		else if (a == "-H" || a == "--Highest-count") O.cs = atol(need(i).c_str());
		else if (a == "-f" || a == "--filter-modulo") { O.f = atol(need(i).c_str()); if (O.f < 1) die("-f must be positive"); }
		else if (a == "-e" || a == "--edit-script-mult") O.cost_mult = atof(need(i).c_str());
		else if (a == "-r" || a == "--max-recurence-level") O.max_rec = atol(need(i).c_str());
		else if (a == "--min-to-alt") O.min_to_alt = atol(need(i).c_str());
		else if (a == "--min-mmer-frac") O.frac_min = atof(need(i).c_str());
		else if (a == "--min-mmer-force-enc") O.frac_always = atof(need(i).c_str());
		else if (a == "--max-matches-mult") O.max_matches_mult = atof(need(i).c_str());
		else if (a == "--min-anchors") O.min_anchors = atol(need(i).c_str());
		else if (a == "-R" || a == "--Ref-reads-mode") { const std::string v = need(i); O.ref_mode = v == "all" ? 0 : v == "sparse" ? 1 : -1; if (O.ref_mode < 0) die("unknown reference reads mode " + v); }
		else if (a == "-g" || a == "--sparse-range") O.g = atof(need(i).c_str());
		else if (a == "-x" || a == "--sparse-exponent") O.exponent = atof(need(i).c_str());
		else if (a == "-t" || a == "--threads") (void)need(i);
		else if (a == "--fill-factor-filtered-kmers" || a == "--fill-factor-kmers-to-reads") (void)need(i);     // host hash-table tuning of the reference: no counterpart here
		else if (a == "-v" || a == "--verbose") O.verbose = true;
		else if (a == "-G" || a == "--reference-genome") O.genome = need(i);
		else if (a == "-s" || a == "--store-reference") O.store_genome = true;
		else if (a == "--gpu") O.gpu = atoi(need(i).c_str());
		else if (a == "--gpus") { O.gpus = atoi(need(i).c_str()); if (O.gpus < 1 || O.gpus > 64) die("--gpus must be in [1, 64]"); }
		else if (a == "--domains") { O.domains = atoi(need(i).c_str()); if (O.domains < 1 || O.domains > 1024) die("--domains must be in [1, 1024]"); }
		else if (a == "--gpu-list") { for (uint32_t v : list_u32(need(i))) O.gpu_list.push_back((int)v); }
		else if (a == "--transport") { O.transport = need(i); if (O.transport != "rccl" && O.transport != "host") die("--transport must be rccl or host"); }
		else if (a == "--chunk-bases") { O.chunk_bases = atof(need(i).c_str()); O.chunk_bases_set = true; }
		else if (a == "--part-symbols") { O.part_symbols = strtoull(need(i).c_str(), nullptr, 10); if (O.part_symbols < 1024 || O.part_symbols > (2u << 21)) die("--part-symbols must be in [1024, 4194304]"); }
		else if (a == "--qual-domain-symbols") { O.qual_domain_symbols = strtoull(need(i).c_str(), nullptr, 10); if (O.qual_domain_symbols < 1) die("--qual-domain-symbols must be positive"); }
		else if (a == "--stream-input") O.stream_input = true;
		else if (a == "--verify-scripts") O.verify_scripts = true;
		else if (a == "--verify-streams") O.verify_streams = true;
		else if (a == "--digest") O.digest = true;
		else if (a == "--digest-values") O.digest = O.digest_values = true;
		else if (a == "--report") O.report = true;
		else if (a == "--edit-profile") O.edit_profile = true;
		else if (a == "--kmer-spectrum") O.kmer_spectrum = true;
		else if (a == "--sketch") O.sketch = true;
		else if (a == "--sketch-size") { O.sketch_size = atol(need(i).c_str()); if (O.sketch_size < 1 || O.sketch_size > (1l << 20)) die("--sketch-size must be in [1, 1048576]"); }
		else if (a == "--sketch-min-count") { O.sketch_min_count = atol(need(i).c_str()); if (O.sketch_min_count < 1 || O.sketch_min_count > 0x7fffffffl) die("--sketch-min-count must be in [1, 2147483647]"); }
		else if (a == "--overlaps") O.overlaps = true;
		else if (a == "--mappings") O.mappings = true;
		else if (a == "--cigars") O.cigars = true;
		else if (a == "--cigars-coded") O.cigars_coded = true;
		else if (a == "--pileup") O.pileup = true;
		else if (a == "--pileup-min-depth") { O.pileup_min_depth = atol(need(i).c_str()); if (O.pileup_min_depth < 0 || O.pileup_min_depth > 0x7fffffffl) die("--pileup-min-depth must be in [0, 2147483647]"); }
		else if (a == "--pileup-min-alt") { O.pileup_min_alt = atol(need(i).c_str()); if (O.pileup_min_alt < 0 || O.pileup_min_alt > 0x7fffffffl) die("--pileup-min-alt must be in [0, 2147483647]"); }
		else if (a == "--pileup-min-frac") { char* e = nullptr; const std::string v = need(i); O.pileup_min_frac = strtod(v.c_str(), &e); if (v.empty() || *e || !(O.pileup_min_frac >= 0 && O.pileup_min_frac <= 1)) die("--pileup-min-frac must be in [0, 1]"); }
		else if (a == "--parse-threads") { O.parse_threads = atoi(need(i).c_str()); if (O.parse_threads < 1 || O.parse_threads > 256) die("--parse-threads must be in [1, 256]"); }
		else if (a == "-h" || a == "--help") { usage(); exit(0); }
		else if (!a.empty() && a[0] == '-' && a.size() > 1) die("unknown option " + a);
		else pos.push_back(a);
	}
	if (pos.size() != 2) { usage(); die("expected input and output paths"); }
	O.in = pos[0]; O.out = pos[1];
	// the checks of arg_parse.cpp:604-625
	if (O.k && !O.a) die("if -k,--kmer-len is set -a,--anchor-len also must be set");
	if (!O.k && O.a) die("if -a,--anchor-len is set -k,--kmer-len also must be set");
	if (O.k && O.a > O.k) die("-a,--anchor-len must be less than or equal to -k,--kmer-len");
	Preset& P = O.P; P = PRESETS[O.source][O.prio];
	auto over = [](uint32_t& dst, long v) { if (v >= 0) dst = (uint32_t)v; };
	over(P.ci, O.ci); over(P.cs, O.cs); over(P.f, O.f); over(P.c, O.c); over(P.max_rec, O.max_rec); over(P.min_part_alt, O.min_to_alt);
	if (O.qual_mode >= 0) P.qual_mode = O.qual_mode;
	if (O.ref_mode >= 0) P.sparse = O.ref_mode;
	if (O.g >= 0) P.g = O.g;
	if (P.c > 64) die("-c,--max-candidates above 64 is not supported by the DNA coder of this build");
	// quality thresholds / representatives (adjust_quality_mode_and_thresholds, arg_parse.cpp:410-450)
	QDef& qd = O.qd; qd = qual_defaults(P.qual_mode);
	const std::string qname = QUAL_MODE_NAMES[P.qual_mode];
	if (O.has_T) { if (qd.fwd.empty()) die("-T,--qual-thresholds is not allowed for '" + qname + "' quality mode"); if (O.T.size() != qd.fwd.size()) die("for '" + qname + "' quality compression mode expected number of quality thresholds is " + std::to_string(qd.fwd.size()) + ", but " + std::to_string(O.T.size()) + " given."); qd.fwd = O.T; }
	if (O.has_D) { if (qd.rev.empty()) die("-D,--qual-values is not allowed for '" + qname + "' quality mode"); if (O.D.size() != qd.rev.size()) die("for '" + qname + "' quality compression mode expected number of quality values is " + std::to_string(qd.rev.size()) + ", but " + std::to_string(O.D.size()) + " given."); qd.rev = O.D; }
	for (size_t i = 0; i < qd.fwd.size(); ++i) if (qd.fwd[i] > 95 || (i && qd.fwd[i] < qd.fwd[i - 1])) die("quality thresholds must be ascending values in [0, 95]");
	if (!O.gpu_list.empty() && O.gpus == 1) O.gpus = (int)O.gpu_list.size();
	if (O.domains > 1 && O.gpus > 1) die("--domains and --gpus exclude each other (every GPU is a model domain already)");
	if (O.stream_input && O.domains > 1) die("--stream-input is not available with --domains");
	if (O.qual_domain_symbols)
	{
		if (O.gpus > 1) die("--qual-domain-symbols is not available with --gpus > 1 (every GPU is a model domain already)");
		if (O.domains > 1) die("--qual-domain-symbols is not available with --domains > 1");
		if (P.qual_mode == 8) die("--qual-domain-symbols needs a coded quality stream: not with -q none (the default of compress-pbraw)");
	}
	if (!O.sketch && (O.sketch_size >= 0 || O.sketch_min_count >= 0)) { usage(); die("--sketch-size and --sketch-min-count need --sketch"); }
	if (O.sketch) { if (O.sketch_size < 0) O.sketch_size = 10000; if (O.sketch_min_count < 0) O.sketch_min_count = 2; }
	if (O.mappings)
	{	// a record's target is a piece of the reference genome, lifted by ONE geometry on ONE device
		if (O.genome.empty()) die("--mappings needs a reference genome (-G): its records are alignments against the genome's pieces");
		if (O.gpus > 1) die("--mappings is not available with --gpus > 1 (the records of the ranks are not merged yet)");
		if (O.domains > 1) die("--mappings is not available with --domains > 1 (every domain is a compressor of its own)");
		if (O.overlaps) die("--mappings is not available with --overlaps (which refuses -G)");
	}
	if (O.cigars && !O.mappings) die("--cigars needs --mappings (with -G): its CIGARs are those of the mapping records");
	if (O.cigars_coded && !O.cigars) die("--cigars-coded needs --cigars (with --mappings and -G): it is a form of their stream");
	if (!O.pileup && (O.pileup_min_depth >= 0 || O.pileup_min_alt >= 0 || O.pileup_min_frac >= 0)) { usage(); die("--pileup-min-depth, --pileup-min-alt and --pileup-min-frac need --pileup"); }
	if (O.pileup)
	{	// a column lies on a piece of the reference genome, placed by ONE geometry in ONE table on ONE device
		if (O.genome.empty()) die("--pileup needs a reference genome (-G): its columns are alignments against the genome's pieces");
		if (O.gpus > 1) die("--pileup is not available with --gpus > 1 (the tables of the ranks are not added yet)");
		if (O.domains > 1) die("--pileup is not available with --domains > 1 (every domain is a compressor of its own)");
		if (O.overlaps) die("--pileup is not available with --overlaps (which refuses -G)");
		if (O.pileup_min_depth < 0) O.pileup_min_depth = 4;
		if (O.pileup_min_alt < 0) O.pileup_min_alt = 3;
		if (O.pileup_min_frac < 0) O.pileup_min_frac = 0.25;
	}
	if (O.overlaps)
	{	// a record names reads of the input: every reference id must be one of them, in ONE set of reference reads
		if (O.gpus > 1) die("--overlaps is not available with --gpus > 1 (the ranks' reference ids are not translated to reads of the input yet)");
		if (O.domains > 1) die("--overlaps is not available with --domains > 1 (every domain has its own reference reads)");
		if (!O.genome.empty()) die("--overlaps is not available with -G (the pseudo reads of a reference genome are no reads of the input)");
	}
	return O;
}
