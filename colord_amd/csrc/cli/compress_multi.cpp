// compress_multi.cpp — `colord_hip compress-* --gpus N | --domains K`: reads sharded over several GPUs, one host thread per GPU (SURVEY.md 8e;
// the reference's orchestrator is one process of threads too, compression.cpp:547-689), built from the steps of compress_common.hpp.  The
// input is read ONCE by the process (gzip and FASTA included): rank r takes the r-th contiguous range of the reads (equal shares of the
// bases), cuts its own reader packs and chunks, and drives its own cl_compressor; the two exchanges of the *_finish steps run through the
// Transport (RCCL, or host staging) bound to cl_exchange; every rank is one model domain of the coders.  Each rank writes ITS parts into the
// archive file at the offsets an all-gather of the byte counts gives it (pwrite; no part travels to another rank); rank 0's thread adds
// `meta`, `header`, `hipdomains`, `hipdigest` (--digest), `info` and the footer.  Also `colord_hip rccl-selftest`.
#include "compress_common.hpp"
#include "transport.hpp"

namespace {
struct Source {                                    // the whole input as records: slices of the mapping (indexed reader) or of one host chunk
	const Reader* R = nullptr; const Chunk* whole = nullptr; uint64_t n = 0;
	uint32_t len(uint64_t i) const { return R->indexed ? R->recs[i].len : (uint32_t)(whole->off[i + 1] - whole->off[i]); }
	const uint8_t* seq(uint64_t i) const { return R->indexed ? R->recs[i].seq : whole->bases + whole->off[i]; }
	const uint8_t* qual(uint64_t i) const { return R->indexed ? R->recs[i].qual : whole->quals + whole->off[i]; }
};
struct RankOut {
	std::vector<uint8_t> dna, qual; std::vector<uint64_t> dsz, qsz; std::vector<uint32_t> counts;      // this rank's parts, in order
	uint64_t n_reads = 0, mean_read_len = 0; uint32_t sparse_range = 0, n_refs = 0; cl_kmer_stats ks{};
	uint64_t dna_base = 0, qual_base = 0, qual_framed = 0;     // where its framed `dna` / `qual` parts start in the file; bytes of the latter
	uint64_t moved = 0;
	std::unique_ptr<cl_kspec> kspec;                           // --kmer-spectrum: what this rank's context counted of the key range it owns (of its own k-mers: an independent domain)
	uint64_t sketch_qualifying = 0; std::vector<cl_sketch_entry> sketch;   // --sketch: the sketch this rank's context made of the key range it owns (of its own k-mers: an independent domain)
	std::unique_ptr<cl_edits> edits;                           // --edit-profile: what this rank's compressor and its lanes counted of their tuple streams
	std::unique_ptr<cl_report> report;                         // --report: what this rank's compressor counted of its reads
	cl_digest dig[3] = { { 0, 0, 0 }, { 0, 0, 0 }, { 0, 0, 0 } }, dig_all[3] = { { 0, 0, 0 }, { 0, 0, 0 }, { 0, 0, 0 } };      // --digest: dna / qual / (--digest-values) qual-values of this rank's reads; of all ranks (as gathered with the byte counts)
};
uint32_t varint_len(uint64_t x) { uint32_t n = 1; for (; x; x >>= 8) ++n; return n; }
}

int run_compress_multi(const Options& O)
{
	const Lap lap{ O.verbose };
	const bool independent = O.domains > 1;             // --domains K: the shares are compressed one after the other on one GPU, nothing is exchanged
	const uint32_t world = independent ? (uint32_t)O.domains : (uint32_t)O.gpus;
	std::vector<int> devs = O.gpu_list;
	if (independent) devs.assign(world, O.gpu);
	if (devs.empty()) for (int i = 0; i < O.gpus; ++i) devs.push_back(i);
	if (devs.size() != world) die("--gpu-list must name --gpus devices");
	int n_dev = 0; hipck(hipGetDeviceCount(&n_dev), "hipGetDeviceCount");
	for (int d : devs) if (d < 0 || d >= n_dev) die("--gpus / --gpu-list: no such device");
	// reference-genome mode (compression.cpp:405-447) with sharded reads: every rank is handed the genome and the pseudo reads, the library
	// lets rank 0 count the genome's k-mers and contribute the pseudo reads (reference reads 0 .. n_pseudo - 1 of the replicated store)
	GenomeMode GM;
	if (!O.genome.empty() && independent) die("-G,--reference-genome is not available with --domains");
	if (!O.genome.empty()) GM.read(O);
	const bool use_rccl = !independent && O.transport == "rccl";
	if (use_rccl) { std::vector<int> u = devs; std::sort(u.begin(), u.end()); if (std::adjacent_find(u.begin(), u.end()) != u.end()) die("--transport rccl needs distinct devices (several ranks on one GPU: --transport host)"); }

	// the input, once
	Reader R; open_reader(O, R);
	Chunk whole; whole.pinned = false;
	Source S; S.R = &R;
	if (R.map && R.index_mapped())
	{
		S.n = R.recs.size();
		for (const auto& r : R.recs) { R.ids.insert(R.ids.end(), r.id, r.id + r.id_len); R.id_off.push_back(R.ids.size()); R.plus.push_back(r.plus_eq); R.n_bases += r.len; }
		R.n_reads = S.n;
	}
	else
	{
		R.indexed = false;
		if (!R.next_chunk(whole, ~0ull >> 1)) die("no reads in " + O.in);
		S.whole = &whole; S.n = whole.off.size() - 1;
	}
	lap("input read");
	const uint64_t n = S.n, total = R.n_bases;
	if (!n) die("no reads in " + O.in);
	if (n >= (1ull << 32)) die("more than 2^32 reads");
	const bool with_qual = R.fastq;
	const KA ka = choose_k_a(O, R);
	const Params prm = make_params(O, ka);

	// shares: rank r starts at the first read whose cumulative base count reaches total * r / world (as colord_amd/mgpu.py)
	std::vector<uint64_t> first(world + 1, n);
	{
		first[0] = 0; uint64_t acc = 0; uint32_t r = 1;
		for (uint64_t i = 0; i < n && r < world; ++i)
		{
			acc += S.len(i);
			while (r < world && (double)acc >= (double)total * r / world) first[r++] = i;
		}
	}
	HeaderCoder hdr; hdr.want_digest = O.digest; hdr.start(R, (uint32_t)n, O.header_mode);
	const bool digest_values = want_digest_values(O, with_qual);
	check_report_options(O, with_qual);

	// transports
	std::vector<std::unique_ptr<Transport>> tp(world);
	RcclGroup rccl; rccl.comms.assign(world, nullptr);
	std::unique_ptr<HostHub> hub;
	if (independent) {}
	else if (use_rccl)
	{
		const ncclResult_t e = ncclCommInitAll(rccl.comms.data(), (int)world, devs.data());
		if (e != ncclSuccess) die(std::string("ncclCommInitAll: ") + ncclGetErrorString(e));
		for (uint32_t r = 0; r < world; ++r) { auto t = std::make_unique<RcclTransport>(); if (t->init(rccl.comms[r], devs[r], r, world, &rccl) != CL_OK) die(t->err); tp[r] = std::move(t); }
	}
	else
	{
		hub = std::make_unique<HostHub>(world);
		for (uint32_t r = 0; r < world; ++r) { auto t = std::make_unique<HostTransport>(); t->init(hub.get(), devs[r], r); tp[r] = std::move(t); }
	}
	const int fd = ::open(O.out.c_str(), O_RDWR | O_CREAT | O_TRUNC, 0644);
	if (fd < 0) die("cannot open file: " + O.out);
	std::vector<RankOut> out(world);
	auto rank_main = [&](uint32_t rank) {
		Transport* const T = tp[rank].get(); RankOut& RO = out[rank];
		hipck(hipSetDevice(devs[rank]), "hipSetDevice");
		cl_ctx* ctx = nullptr; cl_ctx* qctx = nullptr;
		ck(nullptr, cl_ctx_create(devs[rank], &ctx), "cl_ctx_create"); ck(nullptr, cl_ctx_create(devs[rank], &qctx), "cl_ctx_create");
		const uint64_t r0 = first[rank], r1 = first[rank + 1];
		uint64_t my_bases = 0; for (uint64_t i = r0; i < r1; ++i) my_bases += S.len(i);
		cl_exchange X; if (T) X = T->exchange();
		cl_compressor* cmp = nullptr;
		if (O.verify_scripts) cl_ctx_set_verify(ctx, 1);
		if (O.verify_streams) cl_ctx_set_verify_streams(ctx, 1);
		// --digest: a rank's compressor knows its first read in the whole input (exchange 1) and digests its chunks as it encodes them; an independent
		// domain's compressor counts from 0, so its chunks are digested here, at their global read indices, when they first reach the device
		const bool digest_qual = with_qual && O.P.qual_mode != 8;
		if (O.digest && !independent) cl_ctx_set_digest(ctx, 1);
		if (digest_values && !independent) cl_ctx_set_digest_values(ctx, 1);
		if (O.edit_profile) cl_ctx_set_edit_profile(ctx, 1);
		if (O.kmer_spectrum) cl_ctx_set_kmer_spectrum(ctx, 1);
		if (O.sketch) ck(ctx, cl_ctx_set_kmer_sketch(ctx, 1, (uint32_t)O.sketch_size, (uint32_t)O.sketch_min_count), "cl_ctx_set_kmer_sketch");
		if (O.report) cl_ctx_set_report(ctx, 1);                            // (the report has no read indices: a rank's and an independent domain's compressor count alike)
		ck(ctx, cl_compressor_create(ctx, qctx, &prm.cp, with_qual ? &prm.qp : nullptr, T ? &X : nullptr, my_bases, &cmp), "cl_compressor_create");
		if (GM.on) GM.count_kmers(ctx, cmp);
		// chunks of whole reader packs (the packs are cut from this rank's first read on: in_reads.cpp:62-77).  The chunk size follows the
		// rank's share unless --chunk-bases says otherwise: at least 12 chunks a rank, so that the look-ahead pipeline of the compressor (encode
		// lanes, preparation threads: three to five chunks deep) fills — 8 ranks on 5 Gbases would otherwise get one chunk each.
		const uint64_t rank_chunk = O.chunk_bases_set ? (uint64_t)O.chunk_bases : std::min<uint64_t>((uint64_t)O.chunk_bases, std::max<uint64_t>(my_bases / 12, 32ull << 20));
		std::vector<DevChunk> chunks; std::vector<uint64_t> cut;                 // cut[ci] .. cut[ci + 1]: the reads of chunk ci
		Chunk host;
		Reader B; B.part_symbols = O.part_symbols;                            // (its pack / part bookkeeping only)
		// the reads [c0, c1) into the host buffer (offsets, bases, qualities)
		auto fill = [&](uint64_t c0, uint64_t c1) {
			if (host.off.size() != c1 - c0 + 1) { host.clear(); for (uint64_t x = c0; x < c1; ++x) { host.n += S.len(x); host.off.push_back(host.n); } }
			{ const uint64_t tot = host.n; host.n = 0; host.reserve(tot + 1, with_qual); host.n = tot; }
			for (uint64_t x = c0; x < c1; ++x) { memcpy(host.bases + host.off[x - c0], S.seq(x), S.len(x)); if (with_qual) memcpy(host.quals + host.off[x - c0], S.qual(x), S.len(x)); }
		};
		// (cached also where the input is resident: every chunk is released once it is coded, under --stream-input after each of the three
		// passes, and a hipFree each time would stall the lanes and preparation threads of all ranks on the GPU)
		ChunkUploader up(true, with_qual);
		for (uint64_t i = r0; i < r1; )
		{
			host.clear();
			const uint64_t c0 = i;
			while (i < r1 && !host.full(rank_chunk)) { const uint32_t L = S.len(i); host.n += L; host.off.push_back(host.n); B.close_bounds(host, L); ++i; }
			B.finish_bounds(host);
			fill(c0, i);
			DevChunk dc = DevChunk::from(host, with_qual);
			up.upload(ctx, host, dc);
			if (O.digest && independent)
			{
				ck(ctx, cl_digest_bases(ctx, dc.reads, c0, &RO.dig[0]), "content digest");
				if (digest_qual) ck(ctx, cl_digest_quals(ctx, &prm.qp, dc.reads, dc.d_quals, dc.d_off, c0, &RO.dig[1]), "content digest");
				if (digest_values) ck(ctx, cl_digest_qual_values(ctx, &prm.qp, dc.reads, dc.d_quals, dc.d_off, c0, &RO.dig[2]), "content digest");
			}
			ck(ctx, cl_compressor_count_add(cmp, dc.reads), "pass 1");
			if (O.stream_input) up.release(dc);                                 // (--stream-input: a chunk leaves HBM after each pass, as in the single-GPU path)
			cut.push_back(c0);
			chunks.push_back(std::move(dc));
		}
		cut.push_back(r1);
		// a chunk of an earlier pass again (--stream-input): the same reads, from the source this process holds
		auto reload = [&](size_t ci) { host.clear(); fill(cut[ci], cut[ci + 1]); up.upload(ctx, host, chunks[ci]); };
		if (!O.stream_input) host.release();
		ck(ctx, cl_compressor_count_finish(cmp, &RO.ks), "k-mer counting (exchange 1)");
		if (O.kmer_spectrum) { RO.kspec.reset(new cl_kspec); ck(ctx, cl_compressor_kmer_spectrum(cmp, RO.kspec.get()), "cl_compressor_kmer_spectrum"); }
		if (O.sketch)
		{
			cl_sketch* sk = nullptr; uint64_t ns = 0;
			ck(ctx, cl_sketch_create((uint32_t)O.sketch_size, (uint32_t)O.sketch_min_count, &sk), "cl_sketch_create");
			ck(ctx, cl_compressor_kmer_sketch(cmp, sk), "cl_compressor_kmer_sketch");
			ck(ctx, cl_sketch_info(sk, nullptr, nullptr, &RO.sketch_qualifying, &ns), "cl_sketch_info");
			RO.sketch.resize(ns);
			ck(ctx, cl_sketch_entries(sk, RO.sketch.data(), ns), "cl_sketch_entries");
			cl_sketch_free(sk);
		}
		if (GM.on) GM.add_pseudo_reads(ctx, cmp, ka.k);
		for (size_t ci = 0; ci < chunks.size(); ++ci)
		{
			if (O.stream_input) reload(ci);
			ck(ctx, cl_compressor_refs_add(cmp, chunks[ci].reads), "reference reads");
			if (O.stream_input) up.release(chunks[ci]);
		}
		ck(ctx, cl_compressor_refs_finish(cmp), "reference index (exchange 2)");
		ck(ctx, cl_compressor_info(cmp, nullptr, nullptr, nullptr, &RO.mean_read_len, &RO.sparse_range, &RO.n_refs), "cl_compressor_info");
		const OutCaps cap = out_caps(chunks);
		uint8_t* d_dna = nullptr; uint8_t* d_qual = nullptr;
		hipck(hipMalloc((void**)&d_dna, cap.dna), "hipMalloc"); if (with_qual) hipck(hipMalloc((void**)&d_qual, cap.qual), "hipMalloc");
		// --stream-input: the chunks are uploaded again as they are announced and released as they are coded: window + 1 resident, never all
		size_t ann_window = announce_window();
		if (O.stream_input && !ann_window) ann_window = 4;
		size_t announced = 0;
		for (size_t ci = 0; ci < chunks.size(); ++ci)
		{
			DevChunk& dc = chunks[ci];
			for (const size_t have = announce_upto(ann_window, ci, chunks.size()); announced < have; ++announced)
			{
				if (O.stream_input) reload(announced);
				announce(ctx, cmp, chunks[announced]);
			}
			const uint32_t np = (uint32_t)dc.parts.size() - 1;
			std::vector<uint64_t> dsz(np), qsz(np); cl_compress_info info{};
			ck_encode(ctx, cl_compressor_encode(cmp, dc.reads, dc.d_quals, dc.d_off, dc.parts.data(), np, dc.packs.data(), (uint32_t)dc.packs.size() - 1, d_dna, cap.dna, dsz.data(), d_qual, cap.qual, qsz.data(), &info), O.out);
			const size_t od = RO.dna.size(), oq = RO.qual.size();
			RO.dna.resize(od + info.dna_bytes); RO.qual.resize(oq + info.qual_bytes);
			if (info.dna_bytes) hipck(hipMemcpy(RO.dna.data() + od, d_dna, info.dna_bytes, hipMemcpyDeviceToHost), "hipMemcpy");
			if (info.qual_bytes) hipck(hipMemcpy(RO.qual.data() + oq, d_qual, info.qual_bytes, hipMemcpyDeviceToHost), "hipMemcpy");
			RO.dsz.insert(RO.dsz.end(), dsz.begin(), dsz.end()); if (with_qual) RO.qsz.insert(RO.qsz.end(), qsz.begin(), qsz.end());
			for (uint32_t p = 0; p < np; ++p) RO.counts.push_back(dc.parts[p + 1] - dc.parts[p]);
			RO.n_reads += dc.n_reads;
			up.release(dc);
		}
		host.release();
		(void)hipFree(d_dna); if (d_qual) (void)hipFree(d_qual);
		up.clear();
		// where this rank's parts go: an all-gather of the framed byte counts, an exclusive sum, pwrite — `dna` of all ranks first, then `qual`
		if (O.digest && !independent) ck(ctx, cl_compressor_digest(cmp, &RO.dig[0], &RO.dig[1]), "cl_compressor_digest");
		if (digest_values && !independent) ck(ctx, cl_compressor_digest_values(cmp, &RO.dig[2]), "cl_compressor_digest_values");
		if (O.edit_profile) { RO.edits.reset(new cl_edits); ck(ctx, cl_compressor_edit_profile(cmp, RO.edits.get()), "cl_compressor_edit_profile"); }
		if (O.report) { RO.report.reset(new cl_report); ck(ctx, cl_compressor_report(cmp, RO.report.get()), "cl_compressor_report"); }
		// framed bytes of `dna`, `qual`; the content digests travel with them (--digest-values: the fourth triple too, 11 values instead of 8)
		uint64_t mine[11] = { 0, 0, RO.dig[0].reads, RO.dig[0].symbols, RO.dig[0].sum, RO.dig[1].reads, RO.dig[1].symbols, RO.dig[1].sum, RO.dig[2].reads, RO.dig[2].symbols, RO.dig[2].sum };
		const uint32_t n_mine = digest_values ? 11 : 8; const int n_dig = digest_values ? 3 : 2;
		for (size_t p = 0; p < RO.dsz.size(); ++p) mine[0] += varint_len(RO.counts[p]) + RO.dsz[p];
		for (size_t p = 0; p < RO.qsz.size(); ++p) mine[1] += varint_len(0) + RO.qsz[p];
		if (T)
		{
			std::vector<uint64_t> all(n_mine * (size_t)world);
			ck(ctx, T->all_gather_host(mine, n_mine, all.data()), "all-gather of the stream sizes");
			uint64_t dna_all = 0; for (uint32_t r = 0; r < world; ++r) { if (r == rank) RO.dna_base = dna_all; dna_all += all[n_mine * r]; }
			uint64_t q = dna_all; for (uint32_t r = 0; r < world; ++r) { if (r == rank) RO.qual_base = q; q += all[n_mine * r + 1]; }
			for (uint32_t r = 0; r < world; ++r) for (int s = 0; s < n_dig; ++s) { RO.dig_all[s].reads += all[n_mine * r + 2 + 3 * s]; RO.dig_all[s].symbols += all[n_mine * r + 3 + 3 * s]; RO.dig_all[s].sum += all[n_mine * r + 4 + 3 * s]; }
		}
		else
		{	// independent domains run one after the other: a domain's parts follow those of the domains before it
			uint64_t at = 0; for (uint32_t r = 0; r < rank; ++r) at = out[r].qual_base + out[r].qual_framed;
			RO.dna_base = at; RO.qual_base = at + mine[0];
		}
		RO.qual_framed = mine[1];
		auto write_parts = [&](uint64_t at, const std::vector<uint8_t>& data, const std::vector<uint64_t>& sz, bool counted) {
			std::vector<uint8_t> buf; uint64_t o = 0;
			for (size_t p = 0; p < sz.size(); ++p)
			{	// (parts are framed in memory in runs of ~64 MB, one pwrite per run)
				ArchiveWriter::varint(buf, counted ? RO.counts[p] : 0);
				buf.insert(buf.end(), data.begin() + o, data.begin() + o + sz[p]); o += sz[p];
				if (buf.size() >= (64u << 20) || p + 1 == sz.size())
				{
					size_t done = 0;
					while (done < buf.size()) { const ssize_t w = pwrite(fd, buf.data() + done, buf.size() - done, (off_t)(at + done)); if (w <= 0) die("cannot write the archive (disk full?)"); done += (size_t)w; }
					at += buf.size(); buf.clear();
				}
			}
		};
		write_parts(RO.dna_base, RO.dna, RO.dsz, true);
		if (with_qual) write_parts(RO.qual_base, RO.qual, RO.qsz, false);
		RO.moved = T ? T->bytes_moved : 0;
		verified_line(O, cmp, (" (rank " + std::to_string(rank) + ")").c_str());
		cl_compressor_free(cmp);
		cl_ctx_destroy(qctx); cl_ctx_destroy(ctx);
	};
	if (independent) for (uint32_t r = 0; r < world; ++r) rank_main(r);
	else
	{
		std::vector<std::thread> th;
		for (uint32_t r = 0; r < world; ++r) th.emplace_back(rank_main, r);
		for (auto& t : th) t.join();
	}
	lap("all ranks through (parts written)");
	hdr.join(); hdr.check();
	// the rest of the archive behind the parts: meta, header, hipdomains, info, footer — by this thread
	const uint64_t end = out.back().qual_base + out.back().qual_framed;      // (`qual` of the last rank / domain lies last)
	ArchiveWriter ar;
	ar.f = fdopen(fd, "r+b"); if (!ar.f) die("cannot open file: " + O.out);
	if (fseeko(ar.f, (off_t)end, SEEK_SET) != 0) die("cannot seek in the archive");
	ar.off = end;
	const int s_meta = ar.reg("meta"), s_genome = (GM.on && GM.stored) ? ar.reg("ref-genome") : -1, s_header = ar.reg("header"), s_dna = ar.reg("dna"), s_qual = with_qual ? ar.reg("qual") : -1, s_dom = ar.reg("hipdomains");
	const RankOut& R0 = out[0];
	const Totals tot{ (uint32_t)n, total, R0.mean_read_len, R0.sparse_range, ka.k, with_qual };
	add_meta(ar, s_meta, O, GM, tot);
	if (s_genome >= 0) GM.store(ar, s_genome);
	hdr.add_to(ar, s_header);
	// part tables of the streams the ranks wrote, and the model domains (first read, first `dna` part of every rank)
	// (bit 31 of the count: INDEPENDENT domains — each has its own reference reads, so each decodes with a decoder of its own and its
	// own sparse range, appended below; cli/reader.hpp)
	std::vector<uint8_t> dom; le<uint32_t>(dom, world | (independent ? 0x80000000u : 0u));
	uint64_t first_read = 0, dna_total = 0, qual_total = 0;
	for (uint32_t r = 0; r < world; ++r)
	{
		const RankOut& RO = out[r];
		le<uint64_t>(dom, first_read); le<uint64_t>(dom, (uint64_t)ar.streams[s_dna].parts.size());
		uint64_t at = RO.dna_base;
		for (size_t p = 0; p < RO.dsz.size(); ++p) { ar.streams[s_dna].parts.push_back(ArchiveWriter::Part{ at, RO.dsz[p] }); at += varint_len(RO.counts[p]) + RO.dsz[p]; dna_total += RO.dsz[p]; }
		at = RO.qual_base;
		if (with_qual) for (size_t p = 0; p < RO.qsz.size(); ++p) { ar.streams[s_qual].parts.push_back(ArchiveWriter::Part{ at, RO.qsz[p] }); at += 1 + RO.qsz[p]; qual_total += RO.qsz[p]; }
		first_read += RO.n_reads;
	}
	if (first_read != n) die("internal: the ranks' reads do not add up");
	if (independent) for (uint32_t r = 0; r < world; ++r) le<uint32_t>(dom, out[r].sparse_range);
	ar.add(s_dom, dom.data(), dom.size(), 0);
	if (O.digest)
	{	// the ranks' digests added: as rank 0 gathered them with the byte counts, or (independent domains: nothing is exchanged) from the domains' own
		cl_digest dd[3] = { out[0].dig_all[0], out[0].dig_all[1], out[0].dig_all[2] };
		if (independent) for (int s = 0; s < 3; ++s) { dd[s] = cl_digest{ 0, 0, 0 }; for (uint32_t r = 0; r < world; ++r) { dd[s].reads += out[r].dig[s].reads; dd[s].symbols += out[r].dig[s].symbols; dd[s].sum += out[r].dig[s].sum; } }
		if (dd[0].reads != n || dd[0].symbols != total) die("internal: the content digest did not see every read");
		if (digest_values && (dd[2].reads != n || dd[2].symbols != total)) die("internal: the content digest did not see every read");
		add_digest(ar, dd[0], with_qual && O.P.qual_mode != 8 ? &dd[1] : nullptr, hdr.digest, digest_values ? &dd[2] : nullptr);
	}
	if (O.report)
	{	// the ranks' (domains') reports added — they are threads of this process, nothing travels — and the lengths of the one reader for N50 / N90
		ReportSet rep;
		for (uint32_t r = 0; r < world; ++r) if (out[r].report) rp_add(rep.r.get(), out[r].report.get());
		std::vector<uint64_t> lens(n); for (uint64_t i = 0; i < n; ++i) lens[i] = S.len(i);
		add_report(ar, rep, lens, n, total, with_qual && O.P.qual_mode != 8);
	}
	if (O.edit_profile)
	{	// the ranks' (domains') profiles added, as the reports are
		EditsSet E;
		for (uint32_t r = 0; r < world; ++r) if (out[r].edits) ed_add(E.e.get(), out[r].edits.get());
		add_edits(ar, E, n, total);
	}
	if (O.kmer_spectrum)
	{	// ranks own disjoint key ranges of ONE k-mer set (their counters return the sums of all ranks); independent domains are a set each
		KSpecSet K; uint64_t tot_kmers = out[0].ks.tot_kmers, n_unique = out[0].ks.n_unique;
		for (uint32_t r = 0; r < world; ++r) { if (out[r].kspec) ks_add(K.s.get(), out[r].kspec.get()); if (independent && r) { tot_kmers += out[r].ks.tot_kmers; n_unique += out[r].ks.n_unique; } }
		add_kspec(ar, K, prm.cp, GM.on, independent ? world : 1, tot_kmers, n_unique);
	}
	if (O.sketch)
	{	// the merge rule (sketch.hpp): exact over the ranks' disjoint key ranges of ONE k-mer set, and over independent domains, a set each
		cl_sketch* sk = nullptr;
		ck(nullptr, cl_sketch_create((uint32_t)O.sketch_size, (uint32_t)O.sketch_min_count, &sk), "cl_sketch_create");
		for (uint32_t r = 0; r < world; ++r) ck(nullptr, cl_sketch_merge(sk, out[r].sketch.data(), out[r].sketch.size(), out[r].sketch_qualifying), "cl_sketch_merge");
		add_sketch(ar, sk, prm.cp, GM.on, independent ? world : 1);
		cl_sketch_free(sk);
	}
	finish_archive(ar, O, R, tot);
	if (use_rccl) rccl.destroy_all();
	tp.clear();
	whole.release();
	if (R.g) gzclose(R.g);
	fprintf(stderr, "colord_hip: %llu reads, %llu bases on %u GPU(s) [%s], k=%u a=%u; dna %llu B, qual %llu B, header %zu parts; %u reference reads; %llu B exchanged by rank 0; %.2f s\n", (unsigned long long)n, (unsigned long long)total,
		world, use_rccl ? "RCCL" : "host-staged", ka.k, ka.a, (unsigned long long)dna_total, (unsigned long long)qual_total, hdr.parts.size(), R0.n_refs, (unsigned long long)R0.moved, lap.sec());
	return 0;
}

// `colord_hip rccl-selftest [--gpus N]`: the three collectives of RcclTransport on N devices (default 1: a communicator of one rank still runs
// the RCCL code path) with uneven and empty shares, checked against what they must deliver
int run_rccl_selftest(int argc, char** argv)
{
	int world = 1; for (int i = 2; i + 1 < argc; ++i) if (std::string(argv[i]) == "--gpus") world = atoi(argv[i + 1]);
	std::vector<int> devs; for (int i = 0; i < world; ++i) devs.push_back(i);
	std::vector<ncclComm_t> comms((size_t)world, nullptr);
	const ncclResult_t e = ncclCommInitAll(comms.data(), world, devs.data());
	if (e != ncclSuccess) die(std::string("ncclCommInitAll: ") + ncclGetErrorString(e));
	std::vector<std::string> errs((size_t)world);
	auto run = [&](int r) {
		RcclTransport T; if (T.init(comms[r], devs[r], (uint32_t)r, (uint32_t)world) != CL_OK) { errs[r] = T.err; return; }
		auto fillv = [&](uint32_t from, uint32_t to, uint64_t i) { return (uint8_t)(from * 31 + to * 7 + i * 13 + 5); };
		// all_gather_host
		uint64_t v[3] = { (uint64_t)r * 10 + 1, (uint64_t)r * 10 + 2, ~0ull - (uint64_t)r }; std::vector<uint64_t> o(3 * (size_t)world);
		if (T.all_gather_host(v, 3, o.data()) != CL_OK) { errs[r] = T.err; return; }
		for (int p = 0; p < world; ++p) if (o[3 * p] != (uint64_t)p * 10 + 1 || o[3 * p + 2] != ~0ull - (uint64_t)p) { errs[r] = "all_gather_host: wrong values"; return; }
		// all_to_all_v: rank a sends ((a + b) % 3 == 0 ? 0 : 1000 + 17 a + 5 b) bytes to rank b
		auto cnt = [&](int a_, int b_) -> uint64_t { return (a_ + b_) % 3 == 0 && a_ != b_ ? 0ull : 1000ull + 17 * a_ + 5 * b_; };
		std::vector<uint64_t> sb((size_t)world), rb((size_t)world); uint64_t st = 0, rt = 0;
		for (int p = 0; p < world; ++p) { sb[p] = cnt(r, p); rb[p] = cnt(p, r); st += sb[p]; rt += rb[p]; }
		std::vector<uint8_t> hs(st + 1), hr(rt + 1);
		{ uint64_t o2 = 0; for (int p = 0; p < world; ++p) for (uint64_t i = 0; i < sb[p]; ++i) hs[o2++] = fillv((uint32_t)r, (uint32_t)p, i); }
		uint8_t* ds = nullptr; uint8_t* dr = nullptr;
		if (hipMalloc((void**)&ds, st + 1) != hipSuccess || hipMalloc((void**)&dr, rt + 1) != hipSuccess) { errs[r] = "hipMalloc"; return; }
		(void)hipMemcpy(ds, hs.data(), st, hipMemcpyHostToDevice);
		if (T.all_to_all_v(ds, sb.data(), dr, rb.data()) != CL_OK) { errs[r] = T.err; return; }
		(void)hipMemcpy(hr.data(), dr, rt, hipMemcpyDeviceToHost);
		{ uint64_t o2 = 0; for (int p = 0; p < world; ++p) for (uint64_t i = 0; i < rb[p]; ++i) if (hr[o2++] != fillv((uint32_t)p, (uint32_t)r, i)) { errs[r] = "all_to_all_v: wrong bytes"; return; } }
		// all_gather_v: rank a contributes (a % 2 ? 0 : 777 + 3 a) bytes
		auto gc = [&](int a_) -> uint64_t { return a_ % 2 ? 0ull : 777ull + 3 * a_; };
		std::vector<uint64_t> gb((size_t)world); uint64_t gt = 0; for (int p = 0; p < world; ++p) { gb[p] = gc(p); gt += gb[p]; }
		std::vector<uint8_t> gs(gc(r) + 1), gr(gt + 1); for (uint64_t i = 0; i < gc(r); ++i) gs[i] = fillv((uint32_t)r, 99, i);
		uint8_t* dgs = nullptr; uint8_t* dgr = nullptr;
		if (hipMalloc((void**)&dgs, gc(r) + 1) != hipSuccess || hipMalloc((void**)&dgr, gt + 1) != hipSuccess) { errs[r] = "hipMalloc"; return; }
		(void)hipMemcpy(dgs, gs.data(), gc(r), hipMemcpyHostToDevice);
		if (T.all_gather_v(dgs, gc(r), dgr, gb.data()) != CL_OK) { errs[r] = T.err; return; }
		(void)hipMemcpy(gr.data(), dgr, gt, hipMemcpyDeviceToHost);
		{ uint64_t o2 = 0; for (int p = 0; p < world; ++p) for (uint64_t i = 0; i < gb[p]; ++i) if (gr[o2++] != fillv((uint32_t)p, 99, i)) { errs[r] = "all_gather_v: wrong bytes"; return; } }
		(void)hipFree(ds); (void)hipFree(dr); (void)hipFree(dgs); (void)hipFree(dgr);
	};
	std::vector<std::thread> th; for (int r = 0; r < world; ++r) th.emplace_back(run, r);
	for (auto& t : th) t.join();
	for (ncclComm_t c : comms) if (c) (void)ncclCommDestroy(c);
	for (int r = 0; r < world; ++r) if (!errs[r].empty()) die("rccl-selftest, rank " + std::to_string(r) + ": " + errs[r]);
	printf("rccl-selftest: all_gather_host, all_to_all_v, all_gather_v ok on %d rank(s)\n", world);
	return 0;
}
