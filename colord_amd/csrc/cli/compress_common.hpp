// compress_common.hpp — the host steps of runCompression (src/colord/compression.cpp:344-785) that the single-GPU driver (compress.cpp)
// and the sharded one (compress_multi.cpp) share, each once: k / anchor length from the file size, the library's parameters, the reader,
// the reference-genome mode, chunks to the device, look-ahead announcements, the header-coder thread and the `meta` / `info` streams.
#pragma once
#include "colord_hip.h"
#include "options.hpp"
#include "fastx_input.hpp"
#include "genome_io.hpp"
#include "digest_stream.hpp"
#include "report_stream.hpp"
#include "edits_stream.hpp"
#include "overlaps_stream.hpp"
#include "mappings_stream.hpp"
#include "cigars_stream.hpp"
#include "pileup_stream.hpp"
#include "kspec_stream.hpp"
#include "sketch_stream.hpp"
#include <ctime>
#include <mutex>

inline void ck(cl_ctx* ctx, cl_status s, const char* what) { if (s != CL_OK) die(std::string(what) + ": " + (ctx ? cl_last_error(ctx) : "error")); }
// a failed encode call of pass 2 (--verify-scripts: a read that its edit script does not rebuild; --verify-streams: a coded part that does not decode): what is on disk is half a file and goes with the message
inline void ck_encode(cl_ctx* ctx, cl_status s, const std::string& out_path)
{
	if (s == CL_OK) return;
	(void)remove(out_path.c_str());
	die(std::string("pass 2: ") + cl_last_error(ctx) + " (no archive was written)");
}
// -v with --verify-scripts / --verify-streams: what the compressor's contexts checked
inline void verified_line(const Options& O, cl_compressor* cmp, const char* who = "")
{
	uint64_t p = 0, s = 0, n = 0;
	if (O.verify_streams && O.verbose && cl_compressor_verified_streams(cmp, &p, &s, &n) == CL_OK)
		fprintf(stderr, "# coded streams verified%s: %llu parts, %llu symbols, %llu bytes decode to the models' intervals\n", who, (unsigned long long)p, (unsigned long long)s, (unsigned long long)n);
	if (!O.verify_scripts || !O.verbose) return;
	uint64_t r = 0, b = 0;
	if (cl_compressor_verified(cmp, &r, &b) == CL_OK) fprintf(stderr, "# edit scripts verified%s: %llu reads, %llu bases rebuilt on the device and equal to the input\n", who, (unsigned long long)r, (unsigned long long)b);
}
template<class T> void le(std::vector<uint8_t>& v, T x) { for (size_t i = 0; i < sizeof(T); ++i) v.push_back((uint8_t)((uint64_t)x >> (8 * i))); }
inline void le_double(std::vector<uint8_t>& v, double d) { uint64_t u; memcpy(&u, &d, 8); le(v, u); }
// -v: seconds since the start of the run in front of every step
struct Lap {
	bool verbose; std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
	double sec() const { return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count(); }
	void operator()(const char* what) const { if (verbose) fprintf(stderr, "[%7.2f s] %s\n", sec(), what); }
};
// number of bases a file of this size and kind holds, roughly; k / anchor length from it (adjustKmerAndAnchorLen, compression.cpp:42-95)
inline uint64_t estimated_bases(const Reader& R) { return (uint64_t)((R.gz ? (R.fastq ? 2.08 : 3.98) : (R.fastq ? 0.49 : 0.98)) * (double)R.file_bytes); }
struct KA { uint32_t k, a; };
inline KA choose_k_a(const Options& O, const Reader& R)
{
	if (O.k) return { O.k, O.a };
	const uint64_t est = estimated_bases(R);
	return est < 1000000000ull ? KA{ 20, 16 } : est < 4000000000ull ? KA{ 21, 18 } : est < 16000000000ull ? KA{ 23, 21 }
	     : est < 48000000000ull ? KA{ 24, 22 } : est < 128000000000ull ? KA{ 25, 22 } : KA{ 26, 23 };
}
struct Params { cl_compress_params cp{}; cl_qual_params qp{}; };
inline Params make_params(const Options& O, KA ka)
{
	const Preset& P = O.P; Params R; cl_compress_params& cp = R.cp; cl_qual_params& qp = R.qp;
	cp.k = ka.k; cp.f = P.f; cp.ci = P.ci; cp.cs = P.cs; cp.c = P.c; cp.anchor_len = ka.a; cp.min_part_alt = P.min_part_alt; cp.max_rec = P.max_rec; cp.min_anchors = (uint32_t)O.min_anchors;
	cp.level = P.level; cp.source = O.source; cp.sparse = P.sparse; cp.sparse_g = P.g; cp.sparse_exponent = O.exponent;
	cp.cost_mult = O.cost_mult; cp.frac_always = O.frac_always; cp.frac_min = O.frac_min; cp.max_matches_mult = O.max_matches_mult;
	qp.mode = P.qual_mode; qp.source = O.source; qp.level = P.level;
	qp.n_fwd = (uint32_t)O.qd.fwd.size(); std::copy(O.qd.fwd.begin(), O.qd.fwd.end(), qp.fwd);
	qp.n_rev = (uint32_t)O.qd.rev.size(); std::copy(O.qd.rev.begin(), O.qd.rev.end(), qp.rev);
	return R;
}
inline void open_reader(const Options& O, Reader& R)
{
	R.part_symbols = O.part_symbols; R.open(O.in);
	R.threads = O.parse_threads ? O.parse_threads : (int)std::min<unsigned>(32, std::max<unsigned>(1, std::thread::hardware_concurrency()));
	if (const char* e = getenv("COLORD_HIP_PARSE_THREADS")) R.threads = std::max(1, atoi(e));
}

// reference-genome mode (compression.cpp:405-447): the genome's sequences are a second input of the k-mer counter, pieces of them
// ("pseudo reads" of 20 x the mean read length) the first reference reads; the archive holds the genome or its md5
struct GenomeMode {
	bool on = false, stored = false; genome_io::Sequences G, PR; uint32_t read_len = 0, overlap = 0, n_pseudo = 0; std::mutex mu; bool made = false;
	void read(const Options& O)
	{
		on = true; stored = O.store_genome;
		try { G = genome_io::read_fasta(O.genome); } catch (const std::exception& e) { die(e.what()); }
		if (G.off.size() - 1 >= (1ull << 32)) die("reference genome: too many sequences");
		if (O.verbose) fprintf(stderr, "total sequences in reference genome file: %zu (%zu bases)\n", G.off.size() - 1, G.codes.size());
	}
	static cl_reads* upload(cl_ctx* ctx, const genome_io::Sequences& S)
	{
		uint8_t* d_codes = nullptr; uint64_t* d_off = nullptr; cl_reads* r = nullptr;
		hipck(hipMalloc((void**)&d_codes, S.codes.size() + 1), "hipMalloc"); hipck(hipMalloc((void**)&d_off, S.off.size() * 8), "hipMalloc");
		hipck(hipMemcpy(d_codes, S.codes.data(), S.codes.size(), hipMemcpyHostToDevice), "hipMemcpy");
		hipck(hipMemcpy(d_off, S.off.data(), S.off.size() * 8, hipMemcpyHostToDevice), "hipMemcpy");
		ck(ctx, cl_reads_pack(ctx, d_codes, d_off, (uint32_t)(S.off.size() - 1), 0, &r), "reference genome");
		hipck(hipFree(d_codes), "hipFree"); hipck(hipFree(d_off), "hipFree");
		return r;
	}
	void count_kmers(cl_ctx* ctx, cl_compressor* cmp) { cl_reads* gr = upload(ctx, G); ck(ctx, cl_compressor_genome_add(cmp, gr), "reference genome k-mers"); cl_reads_free(gr); }
	// made once (the mean read length is that of ALL reads: the same on every rank of a sharded run)
	void pseudo_reads(uint64_t mean_read_len, uint32_t k)
	{
		std::lock_guard<std::mutex> l(mu);
		if (made) { if (read_len != (uint32_t)(20 * mean_read_len)) die("internal: the ranks disagree about the mean read length"); return; }
		if (20 * mean_read_len >= (1ull << 32)) die("reference genome: pseudo reads too long");
		read_len = (uint32_t)(20 * mean_read_len); overlap = (k - 1) * 10;                      // compression.cpp:407,447
		try { PR = genome_io::pseudo_reads(G, read_len, overlap); } catch (const std::exception& e) { die(e.what()); }
		n_pseudo = (uint32_t)(PR.off.size() - 1);
		made = true;
	}
	void add_pseudo_reads(cl_ctx* ctx, cl_compressor* cmp, uint32_t k)
	{
		uint64_t mrl = 0;
		ck(ctx, cl_compressor_info(cmp, nullptr, nullptr, nullptr, &mrl, nullptr, nullptr), "cl_compressor_info");
		pseudo_reads(mrl, k);
		cl_reads* pr = upload(ctx, PR);
		ck(ctx, cl_compressor_pseudo_reads(cmp, pr), "reference genome pseudo reads");
		cl_reads_free(pr);
	}
	// CReferenceGenome::Store(archive) (reference_genome.cpp:325-370): one part, metadata = number of sequences
	void store(ArchiveWriter& ar, int stream) const
	{
		const uint32_t ns = (uint32_t)(G.off.size() - 1);
		std::vector<uint8_t> gs(G.codes.size() / 3 + 4096); uint64_t got = 0; cl_status st = CL_E_CAPACITY;
		for (int attempt = 0; attempt < 2 && st == CL_E_CAPACITY; ++attempt) { if (attempt) gs.resize(got); st = cl_genome_encode(G.codes.data(), G.off.data(), ns, gs.data(), gs.size(), &got); }
		if (st != CL_OK) die("cannot code the reference genome");
		ar.add(stream, gs.data(), got, ns);
	}
	std::vector<uint64_t> seq_lens() const { std::vector<uint64_t> v; for (size_t s = 0; s + 1 < G.off.size(); ++s) v.push_back(G.off[s + 1] - G.off[s]); return v; }      // the kept bases of every sequence
	void md5(uint8_t md[16]) const { if (cl_genome_md5(G.codes.data(), G.off.data(), (uint32_t)(G.off.size() - 1), md) != CL_OK) die("cannot checksum the reference genome"); }
};

// Device buffers of chunks that come and go (--stream-input, one or several ranks): kept and handed out again instead of a hipMalloc + hipFree
// per chunk — hipFree waits for the WHOLE device, i.e. for the lanes and the preparation working ahead on the chunks after.
struct DevCache {
	std::vector<std::pair<void*, uint64_t>> idle; std::mutex mu;
	void* get(uint64_t bytes, uint64_t& cap)
	{
		std::lock_guard<std::mutex> l(mu);
		size_t best = idle.size();
		for (size_t i = 0; i < idle.size(); ++i) if (idle[i].second >= bytes && (best == idle.size() || idle[i].second < idle[best].second)) best = i;
		if (best != idle.size()) { void* p = idle[best].first; cap = idle[best].second; idle.erase(idle.begin() + (long)best); return p; }
		void* p = nullptr; cap = bytes + bytes / 8 + 4096;                       // (a little room: the chunks are alike, not equal)
		if (hipMalloc(&p, cap) != hipSuccess) { (void)hipGetLastError(); cap = bytes; if (hipMalloc(&p, cap) != hipSuccess) { (void)hipGetLastError(); return nullptr; } }
		return p;
	}
	void put(void* p, uint64_t cap) { std::lock_guard<std::mutex> l(mu); if (p) idle.emplace_back(p, cap); }
	void clear() { std::lock_guard<std::mutex> l(mu); for (auto& x : idle) (void)hipFree(x.first); idle.clear(); }
};
// a chunk of the input on the device: 2-bit arena, quality bytes, offsets; the reader packs and coder parts it is cut into
struct DevChunk {
	cl_reads* reads = nullptr; uint8_t* d_quals = nullptr; uint64_t* d_off = nullptr; std::vector<uint32_t> packs, parts; uint64_t n_bases = 0; uint32_t n_reads = 0; uint64_t quals_cap = 0, off_cap = 0;
	// quality bytes outside 33..128 would index past the coder's tables: the input is rejected, not coded (qualities are Phred+33)
	static DevChunk from(Chunk& host, bool with_qual)
	{
		if (with_qual && !host.quals_in_range()) die("quality values outside '!'..'~'+1 (Phred+33, 0..95) are not supported");
		DevChunk dc; dc.n_reads = (uint32_t)(host.off.size() - 1); dc.n_bases = host.n; dc.packs = host.packs; dc.parts = host.parts;
		return dc;
	}
};
// Host chunk -> DevChunk, one per calling thread.  The 1-byte-per-base form cl_reads_pack reads is needed only during the call: ONE staging
// buffer, kept (a hipMalloc + hipFree per chunk were two device-wide synchronisations in front of every k-mer scan).  `cached`: the chunk's
// own buffers go round through a DevCache instead of a hipMalloc / hipFree each — its own, or another uploader's (`shared`).
struct ChunkUploader {
	const bool cached, with_qual; DevCache own; DevCache& cache;
	uint8_t* stage = nullptr; uint64_t stage_cap = 0; hipStream_t s[2] = { nullptr, nullptr };
	ChunkUploader(bool cached_, bool with_qual_, DevCache* shared = nullptr) : cached(cached_), with_qual(with_qual_), cache(shared ? *shared : own) {}
	~ChunkUploader() { clear(); }
	void clear() { if (stage) (void)hipFree(stage); stage = nullptr; stage_cap = 0; for (hipStream_t& x : s) { if (x) (void)hipStreamDestroy(x); x = nullptr; } own.clear(); }
	void upload(cl_ctx* ctx, const Chunk& host, DevChunk& dc)
	{
		if (host.n + 1 > stage_cap) { if (stage) hipck(hipFree(stage), "hipFree"); stage_cap = host.n + host.n / 8 + 4096; hipck(hipMalloc((void**)&stage, stage_cap), "hipMalloc"); }
		if (cached)
		{
			dc.d_off = (uint64_t*)cache.get(host.off.size() * 8, dc.off_cap); if (with_qual) dc.d_quals = (uint8_t*)cache.get(host.n + 1, dc.quals_cap);
			if (!dc.d_off || (with_qual && !dc.d_quals)) die("out of device memory for a chunk of the input");
		}
		else
		{
			hipck(hipMalloc((void**)&dc.d_off, host.off.size() * 8), "hipMalloc");
			if (with_qual) hipck(hipMalloc((void**)&dc.d_quals, host.n + 1), "hipMalloc (the input does not fit this GPU's memory: --stream-input keeps only a window of it resident)");
		}
		// bases and qualities on a stream each (two copy engines side by side; one after the other they took 91 ms per 2 GB)
		static const bool two_engines = !getenv("COLORD_HIP_UPLOAD_ONE_ENGINE");
		if (two_engines && !s[0]) for (int i = 0; i < 2; ++i) hipck(hipStreamCreateWithFlags(&s[i], hipStreamNonBlocking), "hipStreamCreate");
		auto copy = [&](void* dst, const void* src, uint64_t n, hipStream_t st) {
			if (two_engines) hipck(hipMemcpyAsync(dst, src, n, hipMemcpyHostToDevice, st), "hipMemcpyAsync"); else hipck(hipMemcpy(dst, src, n, hipMemcpyHostToDevice), "hipMemcpy");
		};
		copy(stage, host.bases, host.n, s[0]);
		if (with_qual) copy(dc.d_quals, host.quals, host.n, s[1]);
		hipck(hipMemcpy(dc.d_off, host.off.data(), host.off.size() * 8, hipMemcpyHostToDevice), "hipMemcpy");
		if (two_engines) { hipck(hipStreamSynchronize(s[0]), "hipMemcpyAsync"); hipck(hipStreamSynchronize(s[1]), "hipMemcpyAsync"); }
		ck(ctx, cl_reads_pack(ctx, stage, dc.d_off, dc.n_reads, 1, &dc.reads), "input");        // "Only ACGTN symbols supported inside a read"
	}
	void release(DevChunk& dc)
	{
		if (dc.reads) cl_reads_free(dc.reads);
		if (cached) { cache.put(dc.d_quals, dc.quals_cap); cache.put(dc.d_off, dc.off_cap); }
		else { if (dc.d_quals) (void)hipFree(dc.d_quals); if (dc.d_off) (void)hipFree(dc.d_off); }
		dc.reads = nullptr; dc.d_quals = nullptr; dc.d_off = nullptr;
	}
};
// capacities of the device buffers the `dna` / `qual` parts of any one chunk fit
struct OutCaps { uint64_t dna, qual; };
inline OutCaps out_caps(const std::vector<DevChunk>& chunks)
{
	uint64_t max_bases = 0, max_parts = 0; for (auto& dc : chunks) { max_bases = std::max(max_bases, dc.n_bases); max_parts = std::max<uint64_t>(max_parts, dc.parts.size()); }
	return { max_bases + 64 * max_parts + 4096, (uint64_t)(max_bases * 1.35) + 64 * max_parts + 4096 };
}
// The chunks are announced a window (default 4; 0 = all at once) ahead of the one being coded for the compressor's encode
// lanes and preparation threads to work ahead on; lanes that run far ahead of the coders only pile up edit scripts the pool has to grow for.
inline size_t announce_window() { const char* e = getenv("COLORD_HIP_ANNOUNCE_WINDOW"); return e ? (size_t)std::max(0, atoi(e)) : 4; }
inline size_t announce_upto(size_t window, size_t ci, size_t n_chunks) { return window ? std::min(n_chunks, ci + 1 + window) : n_chunks; }
inline void announce(cl_ctx* ctx, cl_compressor* cmp, const DevChunk& x)
{
	ck(ctx, cl_compressor_prepare_parts(cmp, x.reads, x.packs.data(), (uint32_t)x.packs.size() - 1, x.parts.data(), (uint32_t)x.parts.size() - 1, x.d_quals, x.d_off), "look-ahead");
}

// the `header` stream of ids [0, n) of a reader (CEntrComprHeaders, entr_header.cpp:23-45): packs of >= 4 Mi id bytes (in_reads.cpp:50-56,93-101),
// coded on a host thread of its own, next to the GPU path
struct HeaderCoder {
	std::vector<std::vector<uint8_t>> parts; std::vector<uint32_t> counts; std::string err; std::thread th;
	bool want_digest = false; cl_digest digest{ 0, 0, 0 };                   // --digest: the header digest, on this thread too
	// what `colord_hip decompress` emits for the ids under the archive's -i mode (cl_id_decode_part): org the id and whether the '+' line repeats it,
	// main nothing, none "@"; FASTA has no '+' line
	void digest_headers(const Reader& R, uint32_t n, int header_mode)
	{
		DigestFeed f;
		for (uint32_t i = 0; i < n; ++i)
		{
			if (header_mode == 0) for (uint64_t j = R.id_off[i]; j < R.id_off[i + 1]; ++j) f.push(R.ids[j]);
			else if (header_mode == 2) f.push('@');
			f.push(header_mode == 0 && R.fastq && R.plus[i] ? 1 : 0);
			f.end_read(DG_HEADER);
		}
		digest = f.d;
	}
	void code_headers(const Reader& R, uint32_t n, int header_mode)
	{
		if (want_digest) digest_headers(R, n, header_mode);
		cl_id_coder* idc = nullptr;
		if (cl_id_coder_create(header_mode, &idc) != CL_OK) { err = "cl_id_coder_create"; return; }
		uint32_t i = 0;
		while (i < n)
		{
			uint32_t j = i; uint64_t acc = 0;
			while (j < n) { acc += R.id_off[j + 1] - R.id_off[j]; ++j; if (acc >= (2u << 21)) break; }
			std::vector<uint64_t> off(j - i + 1);
			for (uint32_t t = i; t <= j; ++t) off[t - i] = R.id_off[t] - R.id_off[i];
			std::vector<uint8_t> out(2 * (size_t)off.back() + 64); uint64_t got = 0;
			if (cl_id_encode_part(idc, R.ids.data() + R.id_off[i], off.data(), R.plus.data() + i, j - i, out.data(), out.size(), &got) != CL_OK) { err = cl_id_coder_error(idc); break; }
			out.resize(got); parts.push_back(std::move(out)); counts.push_back(j - i);
			i = j;
		}
		cl_id_coder_free(idc);
	}
	void start(const Reader& R, uint32_t n, int header_mode) { th = std::thread([this, &R, n, header_mode]() { code_headers(R, n, header_mode); }); }
	void join() { th.join(); }
	void check() const { if (!err.empty()) die("header stream: " + err); }
	void add_to(ArchiveWriter& ar, int stream) const { check(); for (size_t p = 0; p < parts.size(); ++p) ar.add(stream, parts[p].data(), parts[p].size(), counts[p]); }
};

// the `meta` stream (compression.cpp:704-779; `info` below: utils.cpp:326-342): one packing for the single- and the multi-GPU host
struct MetaIn { uint32_t n_reads, n_pseudo, tot_ref, c; int level, source; uint64_t mean_read_len; bool with_qual; int qual_mode; std::vector<uint32_t> qual_rev; int header_mode; bool sparse; uint32_t sparse_range; double exponent;
                bool with_genome, store_genome; uint32_t genome_read_len, genome_overlap; const uint8_t* genome_md5; };
inline std::vector<uint8_t> pack_meta(const MetaIn& M)
{
	std::vector<uint8_t> meta;
	le<uint32_t>(meta, M.tot_ref); le<uint32_t>(meta, M.c); le<int32_t>(meta, M.level); meta.push_back((uint8_t)M.source);
	le<uint64_t>(meta, (uint64_t)M.n_reads * M.mean_read_len);
	if (M.with_qual)
	{
		meta.push_back((uint8_t)M.qual_mode);
		if (M.qual_mode == 8 || (M.qual_mode >= 4 && M.qual_mode <= 6)) for (uint32_t v : M.qual_rev) le<uint32_t>(meta, v);
	}
	meta.push_back((uint8_t)M.header_mode);
	meta.push_back(M.sparse ? 1 : 0);                                    // ReferenceReadsMode: All = 0, Sparse = 1
	if (M.sparse) { le<uint32_t>(meta, M.sparse_range); le_double(meta, M.exponent); }
	meta.push_back(M.with_genome ? 1 : 0);                               // compression.cpp:764-777
	if (M.with_genome)
	{
		meta.push_back(M.store_genome ? 1 : 0);
		le<uint32_t>(meta, M.genome_read_len); le<uint32_t>(meta, M.genome_overlap); le<uint32_t>(meta, M.n_pseudo);
		if (!M.store_genome) meta.insert(meta.end(), M.genome_md5, M.genome_md5 + 16);       // the decompressor will ask for the same genome (md5 of its packed sequences)
	}
	return meta;
}
// The tail of an archive.  add_meta: the number of reference reads (all, or those the sparse mode accepts), the genome's md5, `meta`;
// finish_archive: `info` and the footer.  (The drivers add `header`, `ref-genome`, `hipdomains`, `hipdigest` around them in their archives' order.)
struct Totals { uint32_t n_reads; uint64_t n_bases, mean_read_len; uint32_t sparse_range, k; bool with_qual; };
inline void add_meta(ArchiveWriter& ar, int stream, const Options& O, const GenomeMode& GM, const Totals& T)
{
	const Preset& P = O.P;
	uint32_t tot_ref = T.n_reads + GM.n_pseudo;
	if (P.sparse) { std::vector<uint8_t> acc((size_t)T.n_reads + GM.n_pseudo); ck(nullptr, cl_ref_accept(T.n_reads, GM.n_pseudo, T.sparse_range, O.exponent, acc.data()), "cl_ref_accept"); tot_ref = 0; for (uint8_t x : acc) tot_ref += x; }
	uint8_t md[16] = { 0 };
	if (GM.on && !GM.stored) GM.md5(md);
	const std::vector<uint8_t> meta = pack_meta(MetaIn{ T.n_reads, GM.n_pseudo, tot_ref, P.c, P.level, O.source, T.mean_read_len, T.with_qual, P.qual_mode, O.qd.rev, O.header_mode, P.sparse != 0, T.sparse_range, O.exponent,
	                                                    GM.on, GM.stored, GM.read_len, (T.k - 1) * 10, md });
	ar.add(stream, meta.data(), meta.size(), 0);
}
// --digest-values: whether this run digests quality values (cl_ctx_set_digest_values).  Without a coded quality stream (-q none, FASTA
// input) there are none and the run is a plain --digest one: a version-1 stream.
inline bool want_digest_values(const Options& O, bool with_qual)
{
	if (!O.digest_values) return false;
	if (!with_qual || O.P.qual_mode == 8)
	{
		if (O.verbose) fprintf(stderr, "# --digest-values: no coded quality stream (%s): the archive gets the three digests of --digest (`hipdigest` version 1)\n", with_qual ? "-q none" : "the input has no qualities");
		return false;
	}
	for (uint32_t v : O.qd.rev) if (v > 222) die("--digest-values: a -D value above 222 does not fit the quality byte the decoder writes");
	return true;
}
// --digest: the `hipdigest` stream (digest_stream.hpp), before finish_archive; qual: null without a quality stream or in mode none
// values (--digest-values, and only with qual): the qual-values digest, which makes the stream version 2
inline void add_digest(ArchiveWriter& ar, const cl_digest& dna, const cl_digest* qual, const cl_digest& header, const cl_digest* values = nullptr)
{
	DigestSet S; S.flags = 1u | (qual ? 2u : 0u) | 4u | (qual && values ? 8u : 0u); S.d[0] = dna; if (qual) S.d[1] = *qual; S.d[2] = header; if (qual && values) S.d[3] = *values;
	const std::vector<uint8_t> b = S.pack();
	ar.add(ar.reg("hipdigest"), b.data(), b.size(), 0);
}
// --report: the `hipreport` stream (report_stream.hpp), before finish_archive: the additive part as the compressors' contexts counted it, N50 / N90
// from the read lengths the reader saw; what was counted must be every read of the input
inline void add_report(ArchiveWriter& ar, ReportSet& S, const std::vector<uint64_t>& lens, uint64_t n_reads, uint64_t n_bases, bool coded_quals)
{
	const cl_report& r = *S.r;
	if (r.reads != n_reads || r.bases != n_bases || lens.size() != n_reads || (coded_quals && (r.q_reads != n_reads || r.q_symbols != n_bases)) || (!coded_quals && r.has_qual))
		die("internal: the content report did not see every read");
	S.n50 = rp_nxx(lens, 50); S.n90 = rp_nxx(lens, 90);
	const std::vector<uint8_t> b = S.pack();
	ar.add(ar.reg("hipreport"), b.data(), b.size(), 0);
}
// --edit-profile: the `hipedits` stream (edits_stream.hpp), before finish_archive: what the compressors' contexts and their lanes counted of the tuple
// streams; it must be every read of the input
inline void add_edits(ArchiveWriter& ar, const EditsSet& S, uint64_t n_reads, uint64_t n_bases)
{
	if (S.e->reads != n_reads || S.e->bases != n_bases) die("internal: the edit profile did not see every read");
	const std::vector<uint8_t> b = S.pack();
	ar.add(ar.reg("hipedits"), b.data(), b.size(), 0);
}
// --kmer-spectrum: the `hipkmers` stream (kspec_stream.hpp), before finish_archive: what the compressors' contexts counted of the k-mers of pass 1,
// `sets` independent sets added; it must be every k-mer the counters reported
inline void add_kspec(ArchiveWriter& ar, KSpecSet& S, const cl_compress_params& cp, bool genome, uint32_t sets, uint64_t tot_kmers, uint64_t n_unique)
{
	if (S.s->kmers != tot_kmers || S.s->distinct != n_unique) die("internal: the k-mer spectrum did not see every k-mer");
	S.flags = genome ? 1u : 0u; S.k = cp.k; S.f = cp.f; S.ci = cp.ci; S.cs = cp.cs; S.sets = sets;
	const std::vector<uint8_t> b = S.pack();
	ar.add(ar.reg("hipkmers"), b.data(), b.size(), 0);
}
// --overlaps: the `hipoverlaps` stream (overlaps_stream.hpp), before finish_archive: the records the compressor's context and its lanes kept, in
// input order; every record must name reads of the input
inline void add_overlaps(ArchiveWriter& ar, const OverlapSet& S, uint64_t n_reads)
{
	for (const cl_overlap& o : S.recs) if (o.q >= n_reads || o.t >= n_reads) die("internal: an overlap record names a read outside the input");
	const std::vector<uint8_t> b = S.pack();
	ar.add(ar.reg("hipoverlaps"), b.data(), b.size(), 0);
}
// --sketch: the `hipsketch` stream (sketch_stream.hpp), before finish_archive: the sketch the compressors' contexts made of the k-mers of pass 1, `sets`
// independent sets merged
inline void add_sketch(ArchiveWriter& ar, const cl_sketch* sk, const cl_compress_params& cp, bool genome, uint32_t sets)
{
	SketchSet S; uint64_t n = 0;
	if (cl_sketch_info(sk, &S.size, &S.min_count, &S.qualifying, &n) != CL_OK) die("internal: no k-mer sketch");
	S.e.resize(n);
	if (cl_sketch_entries(sk, S.e.data(), n) != CL_OK) die("internal: no k-mer sketch");
	S.flags = genome ? 1u : 0u; S.k = cp.k; S.f = cp.f; S.sets = sets;
	const std::vector<uint8_t> b = S.pack();
	ar.add(ar.reg("hipsketch"), b.data(), b.size(), 0);
}
// --mappings: the `hipmappings` stream (mappings_stream.hpp), before finish_archive: the geometry, the genome's sequence names and lengths, and the
// records the compressor's context and its lanes kept, in input order; every record must name a read of the input and lie on its sequence
inline void add_mappings(ArchiveWriter& ar, MappingSet& S, const GenomeMode& GM, const std::string& genome_path, uint64_t n_reads)
{
	S.read_len = GM.read_len; S.overlap = GM.overlap; S.seq_len = GM.seq_lens();
	try { S.names = genome_io::read_fasta_names(genome_path); } catch (const std::exception& e) { die(e.what()); }
	if (S.names.size() != S.seq_len.size()) die("internal: the reference genome has " + std::to_string(S.seq_len.size()) + " sequences and " + std::to_string(S.names.size()) + " names");
	for (const cl_overlap& o : S.recs) if (o.q >= n_reads || o.t >= S.seq_len.size() || o.te > S.seq_len[o.t] || !(o.flags & OV_GENOME)) die("internal: a mapping record names a read outside the input or lies outside its sequence");
	const std::vector<uint8_t> b = S.pack();
	ar.add(ar.reg("hipmappings"), b.data(), b.size(), 0);
}
// --cigars: the `hipcigars` stream (cigars_stream.hpp), before finish_archive: the CIGARs the compressor's context and its lanes kept, in the order
// of the mapping records S; what is written is what the reader will accept
// coded (--cigars-coded): the record counts and the segments the device coded (version 2); the writer decodes what it wrote, into G.  Returns the stream's bytes.
inline size_t add_cigars(ArchiveWriter& ar, cl_ctx* ctx, cl_compressor* cmp, const MappingSet& S, CigarSet& G, bool coded)
{
	uint64_t nr = 0, no = 0;
	if (coded)
	{
		uint64_t nb = 0, ns = 0;
		const cl_status s = cl_compressor_cigars_coded(cmp, nullptr, 0, &nr, nullptr, 0, &nb, &no, &ns);
		if (s != CL_OK && s != CL_E_CAPACITY) ck(ctx, s, "cl_compressor_cigars_coded");
		std::vector<uint32_t> rec_ops(nr); std::vector<uint8_t> seg(nb);
		if (nr || nb) ck(ctx, cl_compressor_cigars_coded(cmp, rec_ops.data(), nr, &nr, seg.data(), nb, &nb, &no, &ns), "cl_compressor_cigars_coded");
		const std::vector<uint8_t> b = CigarSet::pack_coded(rec_ops, seg, no, ns);
		if (!G.unpack(b, S)) die("internal: the coded CIGARs do not decode to CIGARs that fit the mapping records");
		ar.add(ar.reg("hipcigars"), b.data(), b.size(), 0);
		return b.size();
	}
	const cl_status s = cl_compressor_cigars(cmp, nullptr, 0, &nr, nullptr, 0, &no);
	if (s != CL_OK && s != CL_E_CAPACITY) ck(ctx, s, "cl_compressor_cigars");
	G.rec_ops.resize(nr); G.ops.resize(no);
	if (nr) ck(ctx, cl_compressor_cigars(cmp, G.rec_ops.data(), nr, &nr, G.ops.data(), no, &no), "cl_compressor_cigars");
	const std::vector<uint8_t> b = G.pack();
	CigarSet back;
	if (!back.unpack(b, S)) die("internal: the CIGARs do not fit the mapping records");
	ar.add(ar.reg("hipcigars"), b.data(), b.size(), 0);
	return b.size();
}
// --pileup: the `hippileup` stream (pileup_stream.hpp), before finish_archive: the geometry, the thresholds, the totals of the compressor's table, the genome's
// sequence names and lengths, and the table's sites — the table itself is the size of the genome and stays on the device
inline uint32_t pileup_permille(double frac) { return (uint32_t)(frac * 1000.0 + 0.5); }
inline void add_pileup(ArchiveWriter& ar, cl_ctx* ctx, cl_compressor* cmp, PileupSet& S, const Options& O, const GenomeMode& GM)
{
	cl_pileup* p = nullptr; uint64_t n = 0;
	ck(ctx, cl_compressor_pileup(cmp, &p), "cl_compressor_pileup");
	S.read_len = GM.read_len; S.overlap = GM.overlap; S.seq_len = GM.seq_lens();
	S.thr = PileThresholds{ (uint32_t)O.pileup_min_depth, (uint32_t)O.pileup_min_alt, pileup_permille(O.pileup_min_frac) };
	try { S.names = genome_io::read_fasta_names(O.genome); } catch (const std::exception& e) { die(e.what()); }
	if (S.names.size() != S.seq_len.size()) die("internal: the reference genome has " + std::to_string(S.seq_len.size()) + " sequences and " + std::to_string(S.names.size()) + " names");
	ck(ctx, cl_pileup_totals(p, &S.sums), "cl_pileup_totals");
	const cl_status s = cl_pileup_sites(p, S.thr.min_depth, S.thr.min_alt, S.thr.min_permille, nullptr, 0, &n);
	if (s != CL_OK && s != CL_E_CAPACITY) ck(ctx, s, "cl_pileup_sites");
	S.sites.resize(n);
	if (n) ck(ctx, cl_pileup_sites(p, S.thr.min_depth, S.thr.min_alt, S.thr.min_permille, S.sites.data(), n, &n), "cl_pileup_sites");
	for (const cl_pileup_site& o : S.sites) if (o.seq >= S.seq_len.size() || o.pos >= S.seq_len[o.seq]) die("internal: a pileup site lies outside its sequence");
	const std::vector<uint8_t> b = S.pack();
	ar.add(ar.reg("hippileup"), b.data(), b.size(), 0);
}
// --report with a *-fix mode: the -D values must be qualities the report can index
inline void check_report_options(const Options& O, bool with_qual)
{
	if (!O.report || !with_qual) return;
	if (O.P.qual_mode >= 4 && O.P.qual_mode <= 6) for (uint32_t v : O.qd.rev) if (v > 95) die("--report: a -D value above 95 is no quality the report can count");
}
// `hipqdomains` (--qual-domain-symbols): u64 count, then per model domain of the quality stream its first `qual` part and its first read
inline void add_qual_domains(ArchiveWriter& ar, const std::vector<uint64_t>& first_part, const std::vector<uint64_t>& part_first_read)
{
	std::vector<uint8_t> b; le<uint64_t>(b, first_part.size());
	for (uint64_t p : first_part)
	{
		if (p >= part_first_read.size()) die("internal: a quality model domain starts behind the last part");
		le<uint64_t>(b, p); le<uint64_t>(b, part_first_read[p]);
	}
	ar.add(ar.reg("hipqdomains"), b.data(), b.size(), 0);
}
inline void finish_archive(ArchiveWriter& ar, const Options& O, const Reader& R, const Totals& T)
{
	std::vector<uint8_t> inf;
	le<uint32_t>(inf, 1); le<uint32_t>(inf, 2); le<uint32_t>(inf, 1);                        // archive format of CoLoRd 1.2.1 (defs.h:24-26)
	le<uint64_t>(inf, R.total_bytes); le<uint64_t>(inf, T.n_bases); le<uint32_t>(inf, T.n_reads); le<uint64_t>(inf, (uint64_t)time(nullptr));
	std::string cmd; for (int i = 0; i < O.argc; ++i) { if (i) cmd += ' '; cmd += O.argv[i]; }
	le<uint32_t>(inf, (uint32_t)cmd.size()); inf.insert(inf.end(), cmd.begin(), cmd.end());
	ar.add(ar.reg("info"), inf.data(), inf.size(), 0);
	ar.close();
}
