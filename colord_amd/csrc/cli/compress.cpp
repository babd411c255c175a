// compress.cpp — `colord_hip compress-ont | compress-pbhifi | compress-pbraw [options] input output`: the single-GPU driver, the host side of
// runCompression (src/colord/compression.cpp:344-785).  Options: options.hpp; input parsing: fastx_input.hpp; the steps shared with the
// sharded driver (compress_multi.cpp): compress_common.hpp.  Everything between read bases / qualities and the `dna` / `qual` parts is the
// chunked compressor of the library (cl_compressor_*, csrc/stream.hip): the input is cut in chunks of whole reader packs (--chunk-bases,
// default 1 Gbase) that stay resident in HBM as 2-bit arenas + quality bytes for the three passes, so the file is parsed once and any
// size the GPU holds (~150 Gbases of FASTQ on 288 GB) is one run.
#include "compress_common.hpp"
#include <condition_variable>
#include <deque>
#include <memory>

int run_compress_multi(const Options& O);          // compress_multi.cpp: --gpus N / --domains K

namespace {
// One pass over the input, chunk by chunk: the parser fills one pinned buffer on a thread of its own while the caller works on the other.
struct ChunkPipe {
	Reader& R; const uint64_t chunk_bases; Chunk buf[2]; std::thread prealloc[2]; double t_wait = 0;      // (-v: the callers waiting for the parser)
	// (the two buffers are made, and the HIP runtime started, beside the indexing of the input)
	ChunkPipe(Reader& R_, uint64_t chunk_bases_, int gpu) : R(R_), chunk_bases(chunk_bases_)
	{
		if (!R.map || getenv("COLORD_HIP_NO_PREALLOC")) return;
		const uint64_t est = estimated_bases(R), want = std::min<uint64_t>(chunk_bases, est);
		for (int i = 0; i < (est > want + want / 2 ? 2 : 1); ++i)
			prealloc[i] = std::thread([this, i, want, gpu]() { if (hipSetDevice(gpu) == hipSuccess) buf[i].reserve(want + (8ull << 20), true); });
	}
	void join_prealloc() { for (auto& t : prealloc) if (t.joinable()) t.join(); }
	~ChunkPipe() { join_prealloc(); }
	template<class F> void for_each_chunk(F&& fn)
	{
		std::mutex mu; std::condition_variable cv; int filled[2] = { 0, 0 };      // 0 free, 1 full, 2 end of input
		std::thread parser([&]() {
			for (int i = 0;; i ^= 1)
			{
				{ std::unique_lock<std::mutex> l(mu); cv.wait(l, [&]() { return filled[i] == 0; }); }
				const bool ok = R.next_chunk(buf[i], chunk_bases);
				{ std::lock_guard<std::mutex> l(mu); filled[i] = ok ? 1 : 2; }
				cv.notify_all();
				if (!ok) break;
			}
		});
		for (int hi = 0;; hi ^= 1)
		{
			const auto tw = std::chrono::steady_clock::now();
			{ std::unique_lock<std::mutex> l(mu); cv.wait(l, [&]() { return filled[hi] != 0; }); }
			t_wait += std::chrono::duration<double>(std::chrono::steady_clock::now() - tw).count();
			if (filled[hi] == 2) break;
			fn(buf[hi]);
			{ std::lock_guard<std::mutex> l(mu); filled[hi] = 0; }
			cv.notify_all();
		}
		parser.join();
	}
};
// a later pass over the input (--stream-input) must see the chunks of the first: chunk ci again (`host`), or the end of the input after ci chunks
void same_chunks(const Chunk* host, const std::vector<DevChunk>& chunks, size_t ci)
{
	const bool same = !host ? ci == chunks.size() : ci < chunks.size() && chunks[ci].n_reads == host->off.size() - 1 && chunks[ci].n_bases == host->n && chunks[ci].packs == host->packs && chunks[ci].parts == host->parts;
	if (!same) die("the input changed between two passes over it (--stream-input)");
}

// The parts of a chunk leave through TWO sets of buffers (device and pinned host) and a writer thread: while chunk i + 1 is coded, chunk
// i's parts are copied out on a stream of their own and added to the archive.  (Copied into pageable memory and written by the coding
// thread itself they cost 0.2 s of the 0.55 s a chunk took at 20 Gbases.)  The pinned side is pass 1's staging where the input is
// resident (`adopt`: it is free by now) and grows on demand otherwise: pinning two sets of the device side's worst-case sizes (4.7 GB at
// 1-Gbase chunks, for the 0.8 GB the parts of two chunks take) cost about a second a run.
struct PartWriter {
	ArchiveWriter& ar; const int s_dna, s_qual; const std::vector<DevChunk>& chunks; const OutCaps cap;
	struct Set { uint8_t* d_dna = nullptr; uint8_t* d_qual = nullptr; uint8_t* h_dna = nullptr; uint8_t* h_qual = nullptr; uint64_t h_dna_cap = 0, h_qual_cap = 0; hipEvent_t ev = nullptr; bool busy = false; } set[2];
	struct Job { size_t ci; int b; std::vector<uint64_t> dsz, qsz; };
	hipStream_t stream = nullptr; std::mutex mu; std::condition_variable cv; std::deque<Job> jobs; bool done = false; std::string err; std::thread th;
	double t_wait = 0, t_writer = 0;                      // (-v: the coding thread waiting for the writer; the writer adding parts)
	PartWriter(ArchiveWriter& ar_, int s_dna_, int s_qual_, const std::vector<DevChunk>& chunks_, Chunk* adopt) : ar(ar_), s_dna(s_dna_), s_qual(s_qual_), chunks(chunks_), cap(out_caps(chunks_))
	{
		hipck(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking), "hipStreamCreate");
		for (int b = 0; b < 2; ++b)
		{
			Set& S = set[b];
			hipck(hipMalloc((void**)&S.d_dna, cap.dna), "hipMalloc");
			if (s_qual >= 0) hipck(hipMalloc((void**)&S.d_qual, cap.qual), "hipMalloc");
			hipck(hipEventCreateWithFlags(&S.ev, hipEventDisableTiming), "hipEventCreate");
			if (!adopt) continue;
			S.h_dna = adopt[b].bases; S.h_dna_cap = adopt[b].bases ? adopt[b].cap : 0;
			S.h_qual = adopt[b].quals; S.h_qual_cap = adopt[b].quals ? adopt[b].cap : 0;
			adopt[b].bases = adopt[b].quals = nullptr; adopt[b].cap = 0;
		}
		th = std::thread([this]() { write_jobs(); });
	}
	void write_jobs()
	{
		for (;;)
		{
			Job j;
			{ std::unique_lock<std::mutex> l(mu); cv.wait(l, [&]() { return done || !jobs.empty(); }); if (jobs.empty()) return; j = std::move(jobs.front()); jobs.pop_front(); }
			Set& S = set[j.b];
			if (err.empty() && hipEventSynchronize(S.ev) != hipSuccess) { (void)hipGetLastError(); err = "copy of the parts to the host failed"; }
			const auto tw0 = std::chrono::steady_clock::now();
			if (err.empty())
			{	// (after a failure nothing more goes into the archive: the jobs are only taken off the queue so that the coding thread is not left waiting)
				const DevChunk& dc = chunks[j.ci]; const uint32_t np = (uint32_t)j.dsz.size();
				uint64_t o = 0; for (uint32_t p = 0; p < np; ++p) { ar.add(s_dna, S.h_dna + o, j.dsz[p], dc.parts[p + 1] - dc.parts[p]); o += j.dsz[p]; }
				o = 0; if (s_qual >= 0) for (uint32_t p = 0; p < np; ++p) { ar.add(s_qual, S.h_qual + o, j.qsz[p], 0); o += j.qsz[p]; }
			}
			{ std::lock_guard<std::mutex> l(mu); S.busy = false; t_writer += std::chrono::duration<double>(std::chrono::steady_clock::now() - tw0).count(); }
			cv.notify_all();
		}
	}
	// the buffer set chunk ci is coded into, once the writer is through with it (chunk ci - 2)
	Set& acquire(size_t ci)
	{
		Set& S = set[ci & 1];
		const auto tw = std::chrono::steady_clock::now();
		std::unique_lock<std::mutex> l(mu); cv.wait(l, [&]() { return !S.busy; }); S.busy = true;
		t_wait += std::chrono::duration<double>(std::chrono::steady_clock::now() - tw).count();
		return S;
	}
	// the parts of chunk ci, coded into its set: to the host on the copy stream, then to the archive by the writer
	void submit(size_t ci, std::vector<uint64_t> dsz, std::vector<uint64_t> qsz, const cl_compress_info& info)
	{
		Set& S = set[ci & 1];
		auto host_room = [](uint8_t*& p, uint64_t& room, uint64_t need) {
			if (need <= room) return;
			if (p) (void)hipHostFree(p);
			room = need + need / 4 + (1ull << 20); p = nullptr;
			hipck(hipHostMalloc((void**)&p, room, hipHostMallocDefault), "hipHostMalloc");
		};
		host_room(S.h_dna, S.h_dna_cap, info.dna_bytes); host_room(S.h_qual, S.h_qual_cap, info.qual_bytes);       // (the set is the writer's no more: awaited in acquire)
		if (info.dna_bytes) hipck(hipMemcpyAsync(S.h_dna, S.d_dna, info.dna_bytes, hipMemcpyDeviceToHost, stream), "hipMemcpyAsync");
		if (info.qual_bytes) hipck(hipMemcpyAsync(S.h_qual, S.d_qual, info.qual_bytes, hipMemcpyDeviceToHost, stream), "hipMemcpyAsync");
		hipck(hipEventRecord(S.ev, stream), "hipEventRecord");
		{ std::lock_guard<std::mutex> l(mu); jobs.push_back(Job{ ci, (int)(ci & 1), std::move(dsz), std::move(qsz) }); }
		cv.notify_all();
	}
	// no more parts: the seconds the writer took for its last ones
	double finish()
	{
		{ std::lock_guard<std::mutex> l(mu); done = true; }
		cv.notify_all();
		const auto tj = std::chrono::steady_clock::now();
		th.join();
		return std::chrono::duration<double>(std::chrono::steady_clock::now() - tj).count();
	}
	void release()
	{
		for (Set& S : set) { (void)hipFree(S.d_dna); if (S.h_dna) (void)hipHostFree(S.h_dna); if (S.d_qual) (void)hipFree(S.d_qual); if (S.h_qual) (void)hipHostFree(S.h_qual); (void)hipEventDestroy(S.ev); }
		(void)hipStreamDestroy(stream);
	}
};

// --stream-input, pass 2: a loader thread (a context and an uploader of its own) parses and uploads the chunks again, at most WINDOW + 1
// resident: the one being coded and WINDOW announced ahead of it for the encode lanes and preparation threads; it releases the coded ones
struct ChunkLoader {
	static constexpr size_t WINDOW = 3;
	ChunkUploader up; cl_ctx* ctx = nullptr; std::mutex mu; std::condition_variable cv; size_t n_loaded = 0, done_upto = 0; std::thread th;
	ChunkLoader(int gpu, ChunkPipe& pipe, std::vector<DevChunk>& chunks, bool with_qual, DevCache& cache) : up(true, with_qual, &cache)
	{
		ck(nullptr, cl_ctx_create(gpu, &ctx), "cl_ctx_create");
		pipe.R.rewind();
		th = std::thread([this, gpu, &pipe, &chunks]() {
			hipck(hipSetDevice(gpu), "hipSetDevice");
			size_t freed = 0;
			auto free_done = [&](size_t upto) { for (; freed < upto; ++freed) up.release(chunks[freed]); };
			size_t ci = 0;
			pipe.for_each_chunk([&](Chunk& host) {
				same_chunks(&host, chunks, ci);
				size_t upto;
				{ std::unique_lock<std::mutex> l(mu); cv.wait(l, [&]() { return ci - done_upto < WINDOW + 1; }); upto = done_upto; }
				free_done(upto);
				up.upload(ctx, host, chunks[ci]);
				++ci;
				{ std::lock_guard<std::mutex> l(mu); n_loaded = ci; }
				cv.notify_all();
			});
			same_chunks(nullptr, chunks, ci);
			{ std::unique_lock<std::mutex> l(mu); cv.wait(l, [&]() { return done_upto == chunks.size(); }); }
			free_done(chunks.size());
		});
	}
	size_t wait_loaded(size_t ci) { std::unique_lock<std::mutex> l(mu); cv.wait(l, [&]() { return n_loaded > ci; }); return n_loaded; }     // chunk ci is on the device: how many are
	void coded(size_t ci) { { std::lock_guard<std::mutex> l(mu); done_upto = ci + 1; } cv.notify_all(); }
	void join() { th.join(); cl_ctx_destroy(ctx); }
};
} // namespace

int run_compress(int argc, char** argv)
{
	const Options O = parse_options(argc, argv);
	if (O.gpus > 1 || O.domains > 1) return run_compress_multi(O);
	const Lap lap{ O.verbose };
	hipck(hipSetDevice(O.gpu), "hipSetDevice");
	Reader R; open_reader(O, R);
	ChunkPipe pipe(R, (uint64_t)O.chunk_bases, O.gpu);
	if (R.map && R.index_mapped()) lap("input indexed");
	const KA ka = choose_k_a(O, R); const uint32_t k = ka.k, a = ka.a;
	cl_ctx* ctx = nullptr; cl_ctx* qctx = nullptr;
	ck(nullptr, cl_ctx_create(O.gpu, &ctx), "cl_ctx_create"); ck(nullptr, cl_ctx_create(O.gpu, &qctx), "cl_ctx_create");
	const Params prm = make_params(O, ka);
	const bool with_qual = R.fastq;
	cl_compressor* cmp = nullptr;
	if (O.verify_scripts) cl_ctx_set_verify(ctx, 1);
	if (O.verify_streams) cl_ctx_set_verify_streams(ctx, 1);
	if (O.digest) cl_ctx_set_digest(ctx, 1);
	const bool digest_values = want_digest_values(O, with_qual);
	if (digest_values) cl_ctx_set_digest_values(ctx, 1);
	check_report_options(O, with_qual);
	if (O.report) cl_ctx_set_report(ctx, 1);
	if (O.edit_profile) cl_ctx_set_edit_profile(ctx, 1);
	if (O.kmer_spectrum) cl_ctx_set_kmer_spectrum(ctx, 1);
	if (O.sketch) ck(ctx, cl_ctx_set_kmer_sketch(ctx, 1, (uint32_t)O.sketch_size, (uint32_t)O.sketch_min_count), "cl_ctx_set_kmer_sketch");
	if (O.overlaps) cl_ctx_set_overlaps(ctx, 1);
	if (O.mappings) cl_ctx_set_mappings(ctx, 1);
	if (O.cigars) ck(ctx, cl_ctx_set_cigars(ctx, 1), "cl_ctx_set_cigars");
	if (O.cigars_coded) ck(ctx, cl_ctx_set_cigars_coded(ctx, 1), "cl_ctx_set_cigars_coded");
	if (O.pileup) cl_ctx_set_pileup(ctx, 1);
	std::vector<uint64_t> report_lens;                         // --report: every read length, as the reader hands the reads over in pass 1 (N50 / N90)
	ck(ctx, cl_compressor_create(ctx, qctx, &prm.cp, with_qual ? &prm.qp : nullptr, nullptr, estimated_bases(R), &cmp), "cl_compressor_create");
	if (O.qual_domain_symbols)
	{
		if (!with_qual) die("--qual-domain-symbols needs a quality stream (the input has none)");
		ck(ctx, cl_compressor_set_qual_domain_symbols(cmp, O.qual_domain_symbols), "cl_compressor_set_qual_domain_symbols");
	}
	GenomeMode GM;
	if (!O.genome.empty()) { GM.read(O); GM.count_kmers(ctx, cmp); }
	// pass 1 while parsing: every chunk goes to HBM (2-bit arena + quality bytes) and stays there for the three passes.
	// --stream-input: a chunk leaves HBM again after each pass and the input is read three times (k-mers; reference reads; coding,
	// where the ChunkLoader keeps a window of chunks resident ahead of the coders) — the reference reads its file twice for the same
	// reason (compression.cpp:432,547-561).
	std::vector<DevChunk> chunks;
	pipe.join_prealloc();
	ChunkUploader up(O.stream_input, with_qual);       // (--stream-input: the window's buffers go round through its cache)
	double t_check = 0, t_upload = 0, t_scan = 0;               // (-v: where this thread's time of the pass went)
	pipe.for_each_chunk([&](Chunk& host) {
		auto t0 = std::chrono::steady_clock::now();
		auto lapse = [&](double& acc) { const auto t = std::chrono::steady_clock::now(); acc += std::chrono::duration<double>(t - t0).count(); t0 = t; };
		DevChunk dc = DevChunk::from(host, with_qual);
		if (O.report) for (size_t i = 0; i + 1 < host.off.size(); ++i) report_lens.push_back(host.off[i + 1] - host.off[i]);
		lapse(t_check);
		up.upload(ctx, host, dc);
		lapse(t_upload);
		ck(ctx, cl_compressor_count_add(cmp, dc.reads), "pass 1");
		lapse(t_scan);
		if (O.stream_input) up.release(dc);
		chunks.push_back(std::move(dc));
	});
	lap("input parsed, uploaded and scanned (pass 1)");        // (the pinned staging of a resident input is used once more: pass 2 receives its parts in it)
	if (O.verbose) fprintf(stderr, "# pass 1, this thread: %.2f s waiting for the parser, %.2f s quality range, %.2f s upload + packing, %.2f s k-mer scan; the parser: %.2f s bookkeeping, %.2f s copies (%d threads)\n",
		pipe.t_wait, t_check, t_upload, t_scan, R.t_book, R.t_copy, R.threads);
	const uint32_t n = (uint32_t)R.n_reads; const uint64_t total = R.n_bases;
	if (!n) die("no reads in " + O.in);
	HeaderCoder hdr; hdr.want_digest = O.digest; hdr.start(R, n, O.header_mode);
	cl_kmer_stats ks{};
	ck(ctx, cl_compressor_count_finish(cmp, &ks), "k-mer counting");
	lap("k-mers counted");

	// reference reads: the genome's pseudo reads, then the chunks
	if (GM.on)
	{
		GM.add_pseudo_reads(ctx, cmp, k);
		if (O.verbose) fprintf(stderr, "# ref genome pseudo reads: %u (length %u, overlap %u)\n", GM.n_pseudo, GM.read_len, GM.overlap);
		if (O.mappings || O.pileup)
		{	// the geometry the pieces were cut by: the library makes them again from it and refuses what does not give exactly the pseudo reads
			const std::vector<uint64_t> sl = GM.seq_lens();
			ck(ctx, cl_compressor_genome_geometry(cmp, sl.data(), (uint32_t)sl.size(), GM.read_len, GM.overlap), "cl_compressor_genome_geometry");
		}
	}
	if (!O.stream_input) for (auto& dc : chunks) ck(ctx, cl_compressor_refs_add(cmp, dc.reads), "reference reads");
	else
	{
		R.rewind();
		size_t ci = 0;
		pipe.for_each_chunk([&](Chunk& host) {
			same_chunks(&host, chunks, ci);
			DevChunk dc; dc.n_reads = chunks[ci].n_reads;
			up.upload(ctx, host, dc);
			ck(ctx, cl_compressor_refs_add(cmp, dc.reads), "reference reads");
			up.release(dc);
			++ci;
		});
		same_chunks(nullptr, chunks, ci);
	}
	ck(ctx, cl_compressor_refs_finish(cmp), "reference index");
	lap("reference reads and index");
	uint64_t mean_read_len = 0; uint32_t sparse_range = 0, n_refs = 0;
	ck(ctx, cl_compressor_info(cmp, nullptr, nullptr, nullptr, &mean_read_len, &sparse_range, &n_refs), "cl_compressor_info");
	if (O.verbose) fprintf(stderr, "k=%u a=%u; %llu k-mers, %llu kept; %u reference reads; sparse range %u\n", k, a, (unsigned long long)ks.tot_kmers, (unsigned long long)ks.n_unique_counted, n_refs, sparse_range);

	ArchiveWriter ar; ar.open(O.out);
	const int s_meta = ar.reg("meta"), s_genome = (GM.on && GM.stored) ? ar.reg("ref-genome") : -1, s_header = ar.reg("header"), s_dna = ar.reg("dna"), s_qual = with_qual ? ar.reg("qual") : -1;
	if (s_genome >= 0) GM.store(ar, s_genome);
	// pass 2: chunk by chunk; the parts of a chunk go to the archive (PartWriter) while the next chunk is coded
	uint64_t dna_total = 0, qual_total = 0; uint32_t n_parts_total = 0;
	std::vector<uint64_t> part_first_read; uint64_t reads_before = 0;       // (--qual-domain-symbols: the first read of every part of the file)
	PartWriter pw(ar, s_dna, s_qual, chunks, O.stream_input ? nullptr : pipe.buf);
	std::unique_ptr<ChunkLoader> loader; if (O.stream_input) loader = std::make_unique<ChunkLoader>(O.gpu, pipe, chunks, with_qual, up.cache);
	const size_t ann_window = announce_window();
	size_t announced = 0; double t_encode = 0;
	auto mem_line = [&](const char* when) { size_t fr = 0, tot = 0; if (O.verbose && hipMemGetInfo(&fr, &tot) == hipSuccess) fprintf(stderr, "# device memory %s: %.1f of %.1f GB free\n", when, fr / 1e9, tot / 1e9); };
	for (size_t ci = 0; ci < chunks.size(); ++ci)
	{
		DevChunk& dc = chunks[ci];
		for (const size_t have = O.stream_input ? loader->wait_loaded(ci) : announce_upto(ann_window, ci, chunks.size()); announced < have; ++announced) announce(ctx, cmp, chunks[announced]);      // (--stream-input: whatever the loader has brought)
		if (ci == 0) { lap("pass 2 set up, chunks announced"); mem_line("before the first chunk of pass 2"); }
		const uint32_t np = (uint32_t)dc.parts.size() - 1;
		std::vector<uint64_t> dsz(np), qsz(np); cl_compress_info info{};
		PartWriter::Set& out = pw.acquire(ci);
		const auto te = std::chrono::steady_clock::now();
		ck_encode(ctx, cl_compressor_encode(cmp, dc.reads, dc.d_quals, dc.d_off, dc.parts.data(), np, dc.packs.data(), (uint32_t)dc.packs.size() - 1, out.d_dna, pw.cap.dna, dsz.data(), out.d_qual, pw.cap.qual, qsz.data(), &info), O.out);
		t_encode += std::chrono::duration<double>(std::chrono::steady_clock::now() - te).count();
		pw.submit(ci, std::move(dsz), std::move(qsz), info);
		dna_total += info.dna_bytes; qual_total += info.qual_bytes; n_parts_total += np;
		for (uint32_t p = 0; p < np; ++p) part_first_read.push_back(reads_before + dc.parts[p]);
		reads_before += dc.n_reads;
		// (a resident chunk stays where it is until the pass is over: hipFree waits for the whole device — the lanes and the preparation
		// working ahead on the next chunks — and nobody needs the room)
		if (O.stream_input) loader->coded(ci);                                                                                // (the loader releases it)
		else { size_t fr = 0, tot = 0; if (hipMemGetInfo(&fr, &tot) == hipSuccess && fr < (48ull << 30)) up.release(dc); }   // (... unless the device is nearly full: the pools of the chunks to come take what this one held)
	}
	const double t_last = pw.finish();
	mem_line("after pass 2");
	if (O.verbose) fprintf(stderr, "# pass 2, this thread: %.2f s in the encode calls, %.2f s waiting for the writer to hand a buffer set back, %.2f s for its last parts; the writer: %.2f s adding parts to the archive\n",
		t_encode, pw.t_wait, t_last, pw.t_writer);
	if (!pw.err.empty()) { (void)remove(O.out.c_str()); die(pw.err + " (no archive was written)"); }     // (what is on disk is half a file: it goes with the error)
	if (O.stream_input) { loader->join(); pipe.buf[0].release(); pipe.buf[1].release(); }
	else if (getenv("COLORD_HIP_FULL_TEARDOWN")) for (DevChunk& dc : chunks) up.release(dc);
	pw.release();
	lap("pass 2 (dna + qual parts written)");
	verified_line(O, cmp);

	// tail: header, meta (compression.cpp:704-779), info (utils.cpp:326-342)
	hdr.join();
	lap("header stream");
	hdr.add_to(ar, s_header);
	const Totals tot{ n, total, mean_read_len, sparse_range, k, with_qual };
	add_meta(ar, s_meta, O, GM, tot);
	if (O.digest)
	{	// what the compressor's encode calls digested of their chunks, and the ids
		cl_digest dd{ 0, 0, 0 }, dq{ 0, 0, 0 };
		ck(ctx, cl_compressor_digest(cmp, &dd, &dq), "cl_compressor_digest");
		if (dd.reads != n || dd.symbols != total) die("internal: the content digest did not see every read");
		cl_digest dv{ 0, 0, 0 };
		if (digest_values)
		{
			ck(ctx, cl_compressor_digest_values(cmp, &dv), "cl_compressor_digest_values");
			if (dv.reads != n || dv.symbols != total) die("internal: the content digest did not see every read");
		}
		add_digest(ar, dd, with_qual && O.P.qual_mode != 8 ? &dq : nullptr, hdr.digest, digest_values ? &dv : nullptr);
	}
	if (O.report)
	{
		ReportSet S;
		ck(ctx, cl_compressor_report(cmp, S.r.get()), "cl_compressor_report");
		add_report(ar, S, report_lens, n, total, with_qual && O.P.qual_mode != 8);
	}
	if (O.edit_profile)
	{
		EditsSet E;
		ck(ctx, cl_compressor_edit_profile(cmp, E.e.get()), "cl_compressor_edit_profile");
		add_edits(ar, E, n, total);
	}
	if (O.kmer_spectrum)
	{
		KSpecSet K;
		ck(ctx, cl_compressor_kmer_spectrum(cmp, K.s.get()), "cl_compressor_kmer_spectrum");
		add_kspec(ar, K, prm.cp, GM.on, 1, ks.tot_kmers, ks.n_unique);
	}
	if (O.sketch)
	{
		cl_sketch* sk = nullptr;
		ck(ctx, cl_sketch_create((uint32_t)O.sketch_size, (uint32_t)O.sketch_min_count, &sk), "cl_sketch_create");
		ck(ctx, cl_compressor_kmer_sketch(cmp, sk), "cl_compressor_kmer_sketch");
		add_sketch(ar, sk, prm.cp, GM.on, 1);
		cl_sketch_free(sk);
	}
	if (O.overlaps)
	{
		OverlapSet V; uint64_t nv = 0;
		const cl_status s = cl_compressor_overlaps(cmp, nullptr, 0, &nv);
		if (s != CL_OK && s != CL_E_CAPACITY) ck(ctx, s, "cl_compressor_overlaps");
		V.recs.resize(nv);
		if (nv) ck(ctx, cl_compressor_overlaps(cmp, V.recs.data(), nv, &nv), "cl_compressor_overlaps");
		add_overlaps(ar, V, n);
		if (O.verbose) fprintf(stderr, "# overlaps: %llu records\n", (unsigned long long)nv);
	}
	if (O.mappings)
	{
		MappingSet V; uint64_t nv = 0;
		const cl_status s = cl_compressor_mappings(cmp, nullptr, 0, &nv);
		if (s != CL_OK && s != CL_E_CAPACITY) ck(ctx, s, "cl_compressor_mappings");
		V.recs.resize(nv);
		if (nv) ck(ctx, cl_compressor_mappings(cmp, V.recs.data(), nv, &nv), "cl_compressor_mappings");
		add_mappings(ar, V, GM, O.genome, n);
		if (O.verbose) fprintf(stderr, "# mappings: %llu records on %zu sequences\n", (unsigned long long)nv, V.seq_len.size());
		if (O.cigars)
		{
			CigarSet G;
			const size_t bytes = add_cigars(ar, ctx, cmp, V, G, O.cigars_coded);
			if (O.verbose) fprintf(stderr, "# cigars: %zu operations of %zu records, %zu bytes%s\n", G.ops.size(), G.rec_ops.size(), bytes, O.cigars_coded ? " (coded)" : "");
		}
	}
	if (O.pileup)
	{
		PileupSet V;
		add_pileup(ar, ctx, cmp, V, O, GM);
		if (O.verbose) fprintf(stderr, "# pileup: %llu sites on %zu sequences, %llu positions with an aligned column, %llu reads on genome pieces\n", (unsigned long long)V.sites.size(), V.seq_len.size(),
			(unsigned long long)V.sums.covered, (unsigned long long)V.sums.reads);
	}
	if (O.qual_domain_symbols)
	{
		uint64_t nd = 0;
		(void)cl_compressor_qual_domains(cmp, nullptr, 0, &nd);
		std::vector<uint64_t> first(nd);
		ck(ctx, cl_compressor_qual_domains(cmp, first.data(), nd, &nd), "cl_compressor_qual_domains");
		add_qual_domains(ar, first, part_first_read);
		if (O.verbose) fprintf(stderr, "# quality model domains: %llu (of %llu symbols or more each but the last)\n", (unsigned long long)nd, (unsigned long long)O.qual_domain_symbols);
	}
	finish_archive(ar, O, R, tot);
	gzclose(R.g);
	lap("archive closed");
	fprintf(stderr, "colord_hip: %u reads, %llu bases, k=%u a=%u, %zu chunk(s); dna %llu B (%u parts), qual %llu B, header %zu parts; %u reference reads; %.2f s\n", n, (unsigned long long)total, k, a,
		chunks.size(), (unsigned long long)dna_total, n_parts_total, (unsigned long long)qual_total, hdr.parts.size(), n_refs, lap.sec());
	// The archive is complete and closed.  What is left is handing back tens of GB of device memory, the pinned staging and the mapping of the
	// input allocation by allocation — 0.4-1.2 s at 20 Gbases for what the end of the process does at once.  COLORD_HIP_FULL_TEARDOWN=1 walks
	// through it (leak checks).
	if (!getenv("COLORD_HIP_FULL_TEARDOWN")) { fflush(nullptr); _exit(0); }
	cl_compressor_free(cmp);
	cl_ctx_destroy(qctx); cl_ctx_destroy(ctx);
	return 0;
}
