// decompress.cpp — `colord_hip decompress in.colord out.fastq|out.fasta`, `colord_hip check in.colord` and `colord_hip info in.colord`: the reference's
// runDecompression (src/colord/decompression.cpp:84-258: the FASTQ / FASTA writers) and runInfo (info.cpp:24-53) on top of the
// record stream of reader.hpp (the library's decoders behind the reference's decompression driver).  FASTA is written when the
// archive has no `qual` stream.  No GPU is needed to decompress.  An archive with a `hipdigest` stream (digest_stream.hpp) is checked
// against it while it is decoded; `check` decodes without writing and prints the digests.
#include "reader.hpp"
#include "edits_stream.hpp"
#include "overlaps_stream.hpp"
#include "mappings_stream.hpp"
#include "cigars_stream.hpp"
#include "pileup_stream.hpp"
#include "kspec_stream.hpp"
#include "sketch_stream.hpp"
#include <hip/hip_runtime.h>
#include <chrono>
#include <ctime>
#include <memory>
#include <algorithm>
using namespace colord_hip_reader;

// the device number of `--gpu N`: digits only
static int gpu_number(const char* v)
{
	char* end = nullptr; const long g = strtol(v, &end, 10);
	if (!*v || *end || v[0] < '0' || v[0] > '9' || g < 0 || g > 1023) die(std::string("--gpu needs a device number, not '") + v + "'");
	return (int)g;
}

// ---- `--gpu N`: the quality stream of an archive with `hipqdomains` decoded on the device -----------------------------------------------
// A batch of whole model domains (reader.hpp collects them behind the DNA thread): the bases go to the device and are packed into an arena
// (cl_reads_pack), the class flags of levels 2 and 3 into the form of cl_es_flags, the payloads back to back; cl_qual_decode_domains decodes
// one domain per lane; the qualities come back into the parts, the symbols (for the content digest) through cl_digest_bytes_host.  Without
// --gpu nothing here runs and no device is initialised.
namespace {
struct DevMem {
	void* p = nullptr;
	explicit DevMem(uint64_t bytes) { if (hipMalloc(&p, std::max<uint64_t>(bytes, 16)) != hipSuccess) { (void)hipGetLastError(); p = nullptr; throw std::runtime_error("device memory for the quality decoder (" + std::to_string(bytes) + " bytes)"); } }
	~DevMem() { if (p) (void)hipFree(p); }
	DevMem(const DevMem&) = delete; DevMem& operator=(const DevMem&) = delete;
	template<class T> T* as() const { return (T*)p; }
	void put(const void* h, uint64_t bytes) { if (bytes && hipMemcpy(p, h, bytes, hipMemcpyHostToDevice) != hipSuccess) throw std::runtime_error("copy to the device"); }
	void get(void* h, uint64_t bytes) const { if (bytes && hipMemcpy(h, p, bytes, hipMemcpyDeviceToHost) != hipSuccess) throw std::runtime_error("copy from the device"); }
};
struct DeviceQualDecoder {
	int gpu = 0; cl_ctx* ctx = nullptr;
	uint64_t batches = 0, domains = 0, max_domains = 0, symbols = 0; double seconds = 0, call_seconds = 0, lane_symbol_seconds = 0;       // (the line on stderr at the end)
	explicit DeviceQualDecoder(int g) : gpu(g) {}
	~DeviceQualDecoder() { if (ctx) cl_ctx_destroy(ctx); }
	void operator()(const cl_qual_params& meta_params, QualBatch& B, cl_digest* acc)
	{
		if (!ctx && (hipSetDevice(gpu) != hipSuccess || cl_ctx_create(gpu, &ctx) != CL_OK)) { ctx = nullptr; throw std::runtime_error("--gpu " + std::to_string(gpu) + ": no such device"); }
		const auto t0 = std::chrono::steady_clock::now();
		cl_qual_params qp = meta_params;
		const uint32_t n_parts = (uint32_t)B.parts.size(), n_reads = (uint32_t)B.n_reads;
		// the batch as one read set: offsets, base codes (class flags taken off), flags, part bounds, payloads
		std::vector<uint64_t> off; off.reserve((size_t)n_reads + 1); off.push_back(0);
		std::vector<uint32_t> bounds(1, 0); std::vector<uint64_t> sizes; uint64_t n_in = 0;
		std::vector<uint8_t> codes(B.n_bases), flags(qp.level > 1 ? B.n_bases : 0);
		uint64_t o = 0;
		for (uint32_t p = 0; p < n_parts; ++p)
		{
			const ReadPart& x = B.parts[p];
			for (size_t r = 0; r + 1 < x.off.size(); ++r) off.push_back(o + x.off[r + 1]);
			for (size_t i = 0; i < x.bases.size(); ++i)
			{
				const uint8_t b = x.bases[i];
				codes[o + i] = (b & 7) > 4 ? 4 : (b & 7);
				if (qp.level > 1) flags[o + i] = (b & 0x80) ? 'A' : (b & 0x40) ? 'M' : ' ';               // basic_coder.h:34-35 -> the classes of cl_es_flags
			}
			o += x.bases.size();
			bounds.push_back((uint32_t)(off.size() - 1));
			sizes.push_back(B.payloads[p].size()); n_in += B.payloads[p].size();
		}
		if (off.size() - 1 != n_reads || o != B.n_bases) throw std::runtime_error("the batch's counts do not fit its parts");
		static const uint32_t NAVG[9] = { 0, 10, 8, 4, 0, 0, 0, 2, 0 };
		const uint32_t navg = NAVG[qp.mode]; const bool per_base = qp.mode <= 6, want_symbols = acc && qp.mode != 8;
		const uint64_t n_syms = (uint64_t)n_reads * navg + (per_base ? B.n_bases : 0);
		DevMem d_codes(B.n_bases), d_off(((uint64_t)n_reads + 1) * 8), d_flags(flags.size()), d_in(n_in), d_quals(B.n_bases), d_syms(want_symbols ? n_syms : 0);
		d_codes.put(codes.data(), B.n_bases); d_off.put(off.data(), off.size() * 8); d_flags.put(flags.data(), flags.size());
		{ uint64_t at = 0; for (uint32_t p = 0; p < n_parts; ++p) { if (hipMemcpy(d_in.as<uint8_t>() + at, B.payloads[p].data(), sizes[p], hipMemcpyHostToDevice) != hipSuccess && sizes[p]) throw std::runtime_error("copy to the device"); at += sizes[p]; } }
		cl_reads* reads = nullptr;
		if (cl_reads_pack(ctx, d_codes.as<uint8_t>(), d_off.as<uint64_t>(), n_reads, 0, &reads) != CL_OK) throw std::runtime_error(std::string("cl_reads_pack: ") + cl_last_error(ctx));
		const auto tc = std::chrono::steady_clock::now();
		const cl_status s = cl_qual_decode_domains(ctx, &qp, reads, qp.level > 1 ? d_flags.as<uint8_t>() : nullptr, d_in.as<uint8_t>(), n_in, bounds.data(), sizes.data(), n_parts,
		                                           B.domain_first.data(), (uint32_t)B.domain_first.size(), 0, d_quals.as<uint8_t>(), d_off.as<uint64_t>(), B.n_bases, want_symbols ? d_syms.as<uint8_t>() : nullptr, want_symbols ? n_syms : 0);
		const double t_call = std::chrono::duration<double>(std::chrono::steady_clock::now() - tc).count();
		cl_reads_free(reads);
		if (s != CL_OK) throw std::runtime_error(cl_last_error(ctx));
		call_seconds += t_call; lane_symbol_seconds += t_call * (double)B.domain_first.size();      // (lanes x seconds, batch by batch: the widths differ)
		std::vector<uint8_t> quals(B.n_bases);
		d_quals.get(quals.data(), B.n_bases);
		o = 0;
		for (ReadPart& x : B.parts) { x.quals.assign(quals.begin() + o, quals.begin() + o + x.bases.size()); o += x.bases.size(); }
		if (want_symbols)
		{
			std::vector<uint8_t> syms(n_syms); std::vector<uint64_t> so((size_t)n_reads + 1);
			d_syms.get(syms.data(), n_syms);
			for (uint64_t r = 0; r <= n_reads; ++r) so[r] = r * navg + (per_base ? off[r] : 0);
			if (cl_digest_bytes_host(2, syms.data(), so.data(), n_reads, B.first_read, acc) != CL_OK) throw std::runtime_error("more reads than the content digest can index");
		}
		++batches; domains += B.domain_first.size(); max_domains = std::max<uint64_t>(max_domains, B.domain_first.size()); symbols += n_syms;
		seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
	}
	void report() const
	{
		if (!batches) return;
		// per lane: a batch's symbols over its lanes x the seconds of its cl_qual_decode_domains call (table set-up, launches and the wait for
		// them; the longest domain of a launch sets its time) — not the packing and the copies around it, which `in all` includes
		fprintf(stderr, "colord_hip: quality stream decoded on GPU %d: %llu model domains in %llu batch(es), at most %llu in flight; %llu symbols, %.2f s in the decode calls (%.0f symbols/s per lane), %.2f s in all with packing and copies\n",
			gpu, (unsigned long long)domains, (unsigned long long)batches, (unsigned long long)max_domains, (unsigned long long)symbols, call_seconds, lane_symbol_seconds > 0 ? (double)symbols / lane_symbol_seconds : 0.0, seconds);
	}
};
} // namespace

int run_info(int argc, char** argv)
{
	bool want_report = false, want_edits = false, want_kspec = false, want_sketch = false, want_overlaps = false, names = false, json = false; std::vector<std::string> pos;
	uint64_t min_block = 0; bool has_min_block = false;
	bool want_mappings = false, summary = false; uint64_t coverage = 0;          // --mappings [--coverage W | --summary [--json]]
	bool want_cigar = false, want_sam = false;                                  // --mappings --cigar | --mappings --sam: the PAF with cg:Z:, SAM (`hipcigars`)
	bool want_pileup = false, vcf = false, has_min_alt = false, has_min_frac = false; uint64_t min_alt = 0; double min_frac = 0;      // --pileup [--min-alt N] [--min-frac F] [--vcf] | --pileup --summary [--json]
	for (int i = 2; i < argc; ++i)
	{
		const std::string a = argv[i];
		if (a == "--overlaps") want_overlaps = true;
		else if (a == "--pileup") want_pileup = true;
		else if (a == "--vcf") vcf = true;
		else if (a == "--min-alt")
		{
			char* end = nullptr;
			if (i + 1 >= argc || !isdigit((unsigned char)argv[i + 1][0])) die("option --min-alt needs a number");
			min_alt = strtoull(argv[++i], &end, 10); has_min_alt = true;
			if (*end) die("option --min-alt needs a number");
		}
		else if (a == "--min-frac")
		{
			char* end = nullptr;
			if (i + 1 >= argc || !argv[i + 1][0]) die("option --min-frac needs a fraction in [0, 1]");
			min_frac = strtod(argv[++i], &end); has_min_frac = true;
			if (*end || !(min_frac >= 0 && min_frac <= 1)) die("option --min-frac needs a fraction in [0, 1]");
		}
		else if (a == "--mappings") want_mappings = true;
		else if (a == "--cigar") want_cigar = true;
		else if (a == "--sam") want_sam = true;
		else if (a == "--summary") summary = true;
		else if (a == "--coverage")
		{
			char* end = nullptr;
			if (i + 1 >= argc || !isdigit((unsigned char)argv[i + 1][0])) die("option --coverage needs a window length");
			coverage = strtoull(argv[++i], &end, 10);
			if (*end || !coverage) die("option --coverage needs a window length of one base or more");
		}
		else if (a == "--names") names = true;
		else if (a == "--min-block")
		{
			char* end = nullptr;
			if (i + 1 >= argc || !isdigit((unsigned char)argv[i + 1][0])) die("option --min-block needs a number");
			min_block = strtoull(argv[++i], &end, 10); has_min_block = true;
			if (*end) die("option --min-block needs a number");
		}
		else if (a == "--report") want_report = true; else if (a == "--edit-profile") want_edits = true; else if (a == "--kmer-spectrum") want_kspec = true; else if (a == "--sketch") want_sketch = true; else if (a == "--json") json = true; else pos.push_back(a);
	}
	const int wanted = (want_report ? 1 : 0) + (want_edits ? 1 : 0) + (want_kspec ? 1 : 0) + (want_sketch ? 1 : 0);
	const bool map_paf = want_mappings && !coverage && !summary;            // the three forms of --mappings: PAF (with --min-block, --names), --coverage W, --summary [--json]
	if (pos.size() != 1 || (json && !wanted && !((want_mappings || want_pileup) && summary)) || wanted + (want_overlaps ? 1 : 0) + (want_mappings ? 1 : 0) + (want_pileup ? 1 : 0) > 1 ||
	    ((names || has_min_block) && !want_overlaps && !map_paf) || (coverage && !want_mappings) || (summary && !want_mappings && !want_pileup) || (coverage && summary) ||
	    ((vcf || has_min_alt || has_min_frac) && (!want_pileup || summary)) || ((want_cigar || want_sam) && (!map_paf || (want_cigar && want_sam))))
	{
		fprintf(stderr, "usage: colord_hip info [--report [--json]] [--edit-profile [--json]] [--kmer-spectrum [--json]] archive.colord\n       colord_hip info --overlaps [--min-block N] [--names] archive.colord\n"
			"       colord_hip info --mappings [--min-block N] [--names] | --mappings --coverage W | --mappings --summary [--json] archive.colord\n"
			"       colord_hip info --mappings --cigar | --mappings --sam [--min-block N] [--names] archive.colord\n"
			"       colord_hip info --pileup [--min-alt N] [--min-frac F] [--vcf] | --pileup --summary [--json] archive.colord\n       colord_hip info --sketch [--json] archive.colord\n");
		return 1;
	}
	const std::string& path = pos[0];
	ArchiveReader ar;
	if (!ar.open(path)) die("cannot open archive: " + path);
	if (want_report)
	{	// the stored content report alone, on stdout: nothing is decoded
		ar.close();
		ReportSet S; const int have = read_hipreport(path, S);
		if (have == 0) die("no content report is stored in this archive (written without --report); `colord_hip check` prints what it decodes to");
		if (have < 0) die("the archive's `hipreport` stream is not one this build reads");
		if (json) print_report_json(stdout, S); else print_report(stdout, S, false);
		return 0;
	}
	if (want_edits)
	{	// the stored edit-operation profile alone, on stdout: nothing is decoded
		ar.close();
		EditsSet E; const int have = read_hipedits(path, E);
		if (have == 0) die("no edit profile is stored in this archive (written without --edit-profile)");
		if (have < 0) die("the archive's `hipedits` stream is not one this build reads");
		if (json) print_edits_json(stdout, E); else print_edits(stdout, E);
		return 0;
	}
	if (want_overlaps)
	{	// the stored overlap records as PAF, on stdout: `dna` and `qual` are not decoded; --names decodes the `header` stream on the host
		ar.close();
		OverlapSet V; const int have = read_hipoverlaps(path, V);
		if (have == 0) die("no overlaps are stored in this archive (written without --overlaps)");
		if (have < 0) die("the archive's `hipoverlaps` stream is not one this build reads");
		std::vector<std::string> ids;
		if (names)
		{
			HeaderCache H; H.decode_all(path);
			if (!H.err.empty()) die("--names: " + H.err);
			for (size_t i = 0; i + 1 < H.off.size(); ++i)
			{	// a read's name: its id up to the first blank, or its index where no id is stored (-i none)
				std::string id((const char*)H.ids.data() + H.off[i], (const char*)H.ids.data() + H.off[i + 1]);
				const size_t cut = id.find_first_of(" \t");
				if (cut != std::string::npos) id.resize(cut);
				ids.push_back(id.empty() ? std::to_string(i) : id);
			}
		}
		if (!print_paf(stdout, V, min_block, names ? &ids : nullptr)) die("the archive's `hipoverlaps` stream names a read the `header` stream does not hold");
		return 0;
	}
	if (want_mappings)
	{	// the stored read-to-genome records, on stdout, as PAF, as a coverage track or as a summary: `dna` and `qual` are not decoded, no GPU is used
		uint64_t n_reads = 0;
		if (summary)
		{	// the reads of the archive, as `colord_hip info` prints them
			std::vector<uint8_t> ib; uint64_t im = 0;
			if (!ar.part(ar.id("info"), 0, ib, im) || ib.size() < 40) die("archive without a readable `info` stream");
			try { n_reads = parse_info(ib).total_reads; } catch (const std::exception& e) { die(e.what()); }
		}
		ar.close();
		MappingSet V; const int have = read_hipmappings(path, V);
		if (have == 0) die("no mappings are stored in this archive (written without -G genome --mappings)");
		if (have < 0) die("the archive's `hipmappings` stream is not one this build reads");
		if (coverage) { print_mappings_coverage(stdout, V, coverage); return 0; }
		if (summary) { print_mappings_summary(stdout, summarize_mappings(V, n_reads), json); return 0; }
		std::vector<std::string> ids;
		if (names)
		{
			HeaderCache H; H.decode_all(path);
			if (!H.err.empty()) die("--names: " + H.err);
			for (size_t i = 0; i + 1 < H.off.size(); ++i)
			{	// a read's name: its id up to the first blank, or its index where no id is stored (-i none)
				std::string id((const char*)H.ids.data() + H.off[i], (const char*)H.ids.data() + H.off[i + 1]);
				const size_t cut = id.find_first_of(" \t");
				if (cut != std::string::npos) id.resize(cut);
				ids.push_back(id.empty() ? std::to_string(i) : id);
			}
		}
		if (want_cigar || want_sam)
		{	// the CIGARs of the records, held against them by the reader
			CigarSet G; const int hc = read_hipcigars(path, V, G);
			if (hc == 0) die("no CIGARs are stored in this archive (written without --mappings --cigars)");
			if (hc < 0) die("the archive's `hipcigars` stream is not one this build reads, or does not fit its `hipmappings` stream");
			if (!(want_sam ? print_mappings_sam : print_mappings_paf_cigar)(stdout, V, G, min_block, names ? &ids : nullptr)) die("the archive's `hipmappings` stream names a read the `header` stream does not hold");
			return 0;
		}
		if (!print_mappings_paf(stdout, V, min_block, names ? &ids : nullptr)) die("the archive's `hipmappings` stream names a read the `header` stream does not hold");
		return 0;
	}
	if (want_pileup)
	{	// the stored sites of the per-position base counts, on stdout, as a table, as a VCF or as a summary: nothing is decoded, no GPU is used
		ar.close();
		PileupSet V; const int have = read_hippileup(path, V);
		if (have == 0) die("no pileup is stored in this archive (written without -G genome --pileup)");
		if (have < 0) die("the archive's `hippileup` stream is not one this build reads");
		const uint64_t permille = (uint64_t)(min_frac * 1000.0 + 0.5);
		if (summary) print_pileup_summary(stdout, V, json); else if (vcf) print_pileup_vcf(stdout, V, min_alt, permille); else print_pileup_table(stdout, V, min_alt, permille);
		return 0;
	}
	if (want_kspec)
	{	// the stored k-mer count spectrum alone, on stdout: nothing is decoded
		ar.close();
		KSpecSet K; const int have = read_hipkmers(path, K);
		if (have == 0) die("no k-mer spectrum is stored in this archive (written without --kmer-spectrum)");
		if (have < 0) die("the archive's `hipkmers` stream is not one this build reads");
		if (json) print_kspec_json(stdout, K); else print_kspec(stdout, K);
		return 0;
	}
	if (want_sketch)
	{	// the stored k-mer sketch alone, on stdout: nothing is decoded
		ar.close();
		SketchSet K; const int have = read_hipsketch(path, K);
		if (have == 0) die("no k-mer sketch is stored in this archive (written without --sketch)");
		if (have < 0) die("the archive's `hipsketch` stream is not one this build reads");
		if (json) print_sketch_json(stdout, K); else print_sketch(stdout, K);
		return 0;
	}
	std::vector<uint8_t> b; uint64_t meta = 0;
	if (!ar.part(ar.id("info"), 0, b, meta) || b.size() < 40) die("archive without a readable `info` stream");
	ArchiveInfo I;
	try { I = parse_info(b); } catch (const std::exception& e) { die(e.what()); }
	time_t t = (time_t)I.time;
	fprintf(stderr, "version major: %u\nversion minor: %u\nversion patch: %u\ntotal bytes: %llu\ntotal bases: %llu\ntotal reads: %u\ntime: %s\ncommand: %s\n",
		I.version_major, I.version_minor, I.version_patch, (unsigned long long)I.total_bytes, (unsigned long long)I.total_bases, I.total_reads, asctime(localtime(&t)), I.command_line.c_str());
	ar.close();
	DigestSet stored;                                                          // archives written with --digest: the content digests they must decode to
	if (read_hipdigest(path, stored) > 0) for (int j = 0; j < 4; ++j) if (const int i = DigestSet::in_order(j); (stored.flags >> i) & 1) fprintf(stderr, "content digest: %s\n", stored.line(i).c_str());
	ReportSet rep;
	if (const int have = read_hipreport(path, rep); have > 0)
		fprintf(stderr, "content report: %llu reads, %llu bases, N50 %llu, %s (`colord_hip info --report [--json]` prints it)\n", (unsigned long long)rep.r->reads, (unsigned long long)rep.r->bases, (unsigned long long)rep.n50,
			rep.r->has_qual ? "input against stored quality values" : "no quality part");
	else if (have < 0) fprintf(stderr, "content report: a `hipreport` stream this build cannot read\n");
	EditsSet eds;
	if (const int have = read_hipedits(path, eds); have > 0)
		fprintf(stderr, "edit profile: %llu of %llu reads coded with an edit script, %llu aligned bases (`colord_hip info --edit-profile [--json]` prints it)\n", (unsigned long long)eds.e->kind_reads[2], (unsigned long long)eds.e->reads,
			(unsigned long long)edits_derived(*eds.e).aligned);
	else if (have < 0) fprintf(stderr, "edit profile: a `hipedits` stream this build cannot read\n");
	KSpecSet ksp;
	if (const int have = read_hipkmers(path, ksp); have > 0)
		fprintf(stderr, "k-mer spectrum: %llu sampled k-mers (1 in %u), %llu distinct, highest count %llu (`colord_hip info --kmer-spectrum [--json]` prints it)\n", (unsigned long long)ksp.s->kmers, ksp.f, (unsigned long long)ksp.s->distinct,
			(unsigned long long)ksp.s->max_count);
	else if (have < 0) fprintf(stderr, "k-mer spectrum: a `hipkmers` stream this build cannot read\n");
	SketchSet skt;
	if (const int have = read_hipsketch(path, skt); have > 0)
		fprintf(stderr, "k-mer sketch: %llu of %llu qualifying k-mers (count >= %u, 1 in %u, k = %u), %s (`colord_hip info --sketch [--json]` prints it, `colord_hip dist` compares archives)\n", (unsigned long long)skt.e.size(),
			(unsigned long long)skt.qualifying, skt.min_count, skt.f, skt.k, skt.complete() ? "complete" : "the lowest hashes");
	else if (have < 0) fprintf(stderr, "k-mer sketch: a `hipsketch` stream this build cannot read\n");
	OverlapSet ovl;
	if (const int have = read_hipoverlaps(path, ovl); have > 0)
		fprintf(stderr, "overlaps: %llu records of reads against reference reads (`colord_hip info --overlaps [--min-block N] [--names]` prints them as PAF)\n", (unsigned long long)ovl.recs.size());
	else if (have < 0) fprintf(stderr, "overlaps: a `hipoverlaps` stream this build cannot read\n");
	MappingSet mps;
	if (const int have = read_hipmappings(path, mps); have > 0)
		fprintf(stderr, "mappings: %llu records of reads against the %zu sequences of the reference genome (`colord_hip info --mappings [--min-block N] [--names]` prints them as PAF, `--mappings --coverage W` a coverage track, `--mappings --summary [--json]` what they add up to)\n",
			(unsigned long long)mps.recs.size(), mps.seq_len.size());
	else if (have < 0) fprintf(stderr, "mappings: a `hipmappings` stream this build cannot read\n");
	uint64_t cg_records = 0, cg_operations = 0; CigarCoded cg_coded;
	if (const int have = peek_hipcigars(path, cg_records, cg_operations, &cg_coded); have > 0)
	{
		fprintf(stderr, "cigars: %llu operations of %llu mapping records", (unsigned long long)cg_operations, (unsigned long long)cg_records);
		if (cg_coded.version == 2) fprintf(stderr, ", coded: %llu bytes in %llu segments, %.3f bytes per operation, %llu escapes", (unsigned long long)cg_coded.bytes, (unsigned long long)cg_coded.segments,
			cg_operations ? (double)cg_coded.bytes / (double)cg_operations : 0.0, (unsigned long long)cg_coded.escapes);
		fprintf(stderr, " (`colord_hip info --mappings --cigar` prints the PAF with cg:Z:, `--mappings --sam` SAM)\n");
	}
	else if (have < 0) fprintf(stderr, "cigars: a `hipcigars` stream this build cannot read\n");
	PileupSet pil;
	if (const int have = read_hippileup(path, pil); have > 0)
		fprintf(stderr, "pileup: %llu sites on the %zu sequences of the reference genome, %llu positions with an aligned column (`colord_hip info --pileup [--min-alt N] [--min-frac F]` prints the sites, `--pileup --vcf` a VCF, `--pileup --summary [--json]` what the table adds up to)\n",
			(unsigned long long)pil.sites.size(), pil.seq_len.size(), (unsigned long long)pil.sums.covered);
	else if (have < 0) fprintf(stderr, "pileup: a `hippileup` stream this build cannot read\n");
	return 0;
}

// `colord_hip dist [--json] A.colord B.colord [C.colord ...]`: A against each of the others by their `hipsketch` streams alone (sketch_stream.hpp); no GPU
int run_dist(int argc, char** argv)
{
	bool json = false; std::vector<std::string> pos;
	for (int i = 2; i < argc; ++i) { const std::string a = argv[i]; if (a == "--json") json = true; else if (a.size() > 1 && a[0] == '-') { pos.clear(); break; } else pos.push_back(a); }
	if (pos.size() < 2) { fprintf(stderr, "usage: colord_hip dist [--json] A.colord B.colord [C.colord ...]\n"); return 1; }
	std::vector<SketchSet> S(pos.size());
	for (size_t i = 0; i < pos.size(); ++i)
	{
		{ ArchiveReader ar; if (!ar.open(pos[i])) die("cannot open archive: " + pos[i]); ar.close(); }
		const int have = read_hipsketch(pos[i], S[i]);
		if (have == 0) die("no k-mer sketch is stored in " + pos[i] + " (written without --sketch)");
		if (have < 0) die("the `hipsketch` stream of " + pos[i] + " is not one this build reads");
		if (S[i].k != S[0].k || S[i].f != S[0].f)
			die("sketches compare at equal k and f only: " + pos[i] + " has k = " + std::to_string(S[i].k) + ", f = " + std::to_string(S[i].f) + ", " + pos[0] + " has k = " + std::to_string(S[0].k) + ", f = " + std::to_string(S[0].f));
	}
	for (size_t i = 0; i < pos.size(); ++i)
	{
		if (i && S[i].min_count != S[0].min_count) fprintf(stderr, "colord_hip: note: %s was sketched with min_count %u, %s with %u: the k-mer sets were cut differently\n", pos[i].c_str(), S[i].min_count, pos[0].c_str(), S[0].min_count);
		if (S[i].sets > 1) fprintf(stderr, "colord_hip: note: %s: %s\n", pos[i].c_str(), SKETCH_SETS_NOTE);
		if (S[i].flags & 1) fprintf(stderr, "colord_hip: note: %s: the k-mers of a reference genome are in the sketch\n", pos[i].c_str());
	}
	// one line per pair: A, B, distance, jaccard, shared, compared, containment_of_A, containment_of_B
	for (size_t i = 1; i < pos.size(); ++i)
	{
		const SketchDist D = sketch_dist(S[0], S[i]);
		if (json)
			printf("{\"a\": \"%s\", \"b\": \"%s\", \"k\": %u, \"f\": %u, \"shared\": %llu, \"compared\": %llu, \"in_a\": %llu, \"in_b\": %llu, \"jaccard\": %.17g, \"containment_of_a\": %.17g, \"containment_of_b\": %.17g, \"distance\": %.17g}\n",
				json_escape(pos[0]).c_str(), json_escape(pos[i]).c_str(), S[0].k, S[0].f, (unsigned long long)D.shared, (unsigned long long)D.compared, (unsigned long long)D.in_a, (unsigned long long)D.in_b, D.jaccard, D.containment_a, D.containment_b, D.distance);
		else
			printf("%s\t%s\t%.17g\t%.17g\t%llu\t%llu\t%.17g\t%.17g\n", pos[0].c_str(), pos[i].c_str(), D.distance, D.jaccard, (unsigned long long)D.shared, (unsigned long long)D.compared, D.containment_a, D.containment_b);
	}
	return 0;
}

// one record as the reference's writers put it out (decompression.cpp:84-258)
static void format_record(std::vector<char>& line, const Record& r, bool is_fastq)
{
	line.clear();
	line.push_back(is_fastq ? '@' : '>');
	line.insert(line.end(), r.header, r.header + r.header_len); line.push_back('\n');
	for (size_t i = 0; i < r.n_bases; ++i) line.push_back("ACGTN"[(r.bases[i] & 7) > 4 ? 4 : (r.bases[i] & 7)]);
	line.push_back('\n');
	if (is_fastq)
	{
		line.push_back('+');
		if (r.plus_is_header) line.insert(line.end(), r.header, r.header + r.header_len);
		line.push_back('\n');
		line.insert(line.end(), r.quals, r.quals + r.n_bases); line.push_back('\n');
	}
}
// what decoding an archive gave: its records, and (asked for) the content digests of what the decoders returned
struct Decoded { uint64_t n_rec = 0; DigestSet computed; size_t domains = 0, at_a_time = 0; bool want_report = false; ReportSet report; std::vector<uint64_t> lens; };

// Archives with INDEPENDENT model domains (`colord_hip compress-* --domains K`): every domain is decoded by a worker of its own — three
// stream threads each, as for a whole archive — into a file of its own next to the output; the files are then joined in order.  The ids
// come from one pass over the `header` stream that all workers share.  false: the archive is not of that kind (the caller then decodes
// it as one stream).  out_path empty: nothing is written (`colord_hip check`).  With want_digest every worker digests its domain's reads
// at their indices in the whole input and the partial digests are added; the header digest is the shared pass's.  want_values: the
// qual-values digest of the quality bytes too.
static bool decode_domains(const std::string& arc, const std::string& genome, const std::string& out_path, int max_threads, bool want_digest, bool want_values, Decoded& D)
{
	size_t K = 0; bool is_fastq = true;
	{ RecordStream probe(arc, genome); if (!probe.independent_domains() || probe.n_domains() < 2) return false; K = probe.n_domains(); is_fastq = probe.is_fastq(); }
	const bool writing = !out_path.empty();
	HeaderCache hc; hc.want_digest = want_digest;
	std::thread ht([&]() { hc.decode_all(arc); });
	std::vector<std::string> errs(K), tmp(K); std::vector<uint64_t> n_rec(K, 0); std::vector<DigestSet> dig(K);
	for (size_t d = 0; d < K; ++d) tmp[d] = out_path + ".domain" + std::to_string(d) + ".tmp";
	// the dna / qual threads of the first `max_threads` domains start at once; the ids are needed from the first record on
	std::mutex mu; size_t next_dom = 0;
	auto worker = [&]() {
		for (;;)
		{
			size_t d; { std::lock_guard<std::mutex> l(mu); if (next_dom >= K) return; d = next_dom++; }
			try
			{
				RecordStream r(arc, genome, (int)d, &hc);
				if (want_digest) r.enable_digest();
				if (want_values) r.enable_digest_values();
				if (D.want_report) r.enable_report();
				r.prefetch();
				{ static std::mutex hm; std::lock_guard<std::mutex> l(hm); if (ht.joinable()) ht.join(); }
				if (!hc.err.empty()) throw std::runtime_error("header stream: " + hc.err);
				FILE* out = writing ? fopen(tmp[d].c_str(), "wb") : nullptr;
				if (writing && !out) throw std::runtime_error("cannot open file: " + tmp[d]);
				std::vector<char> obuf(writing ? 1 << 22 : 1); if (out) setvbuf(out, obuf.data(), _IOFBF, obuf.size());
				std::vector<char> line; Record rec; bool ok = true;
				while (r.next(rec)) { if (out) { format_record(line, rec, is_fastq); if (fwrite(line.data(), 1, line.size(), out) != line.size()) { ok = false; break; } } ++n_rec[d]; }
				if (out && (fflush(out) != 0 || ferror(out))) ok = false;
				if (out && fclose(out) != 0) ok = false;
				if (!ok) throw std::runtime_error("cannot write " + tmp[d] + " (disk full?)");
				if (want_digest) dig[d] = r.digests();
				if (D.want_report) { std::lock_guard<std::mutex> l(mu); r.report_into(D.report, D.lens); }
			}
			catch (const std::exception& e) { errs[d] = e.what(); }
		}
	};
	const size_t T = std::min<size_t>(K, (size_t)std::max(1, max_threads));
	std::vector<std::thread> th; for (size_t i = 0; i < T; ++i) th.emplace_back(worker);
	for (auto& t : th) t.join();
	if (ht.joinable()) ht.join();
	for (size_t d = 0; d < K; ++d) if (!errs[d].empty()) { if (writing) for (auto& t : tmp) remove(t.c_str()); die("domain " + std::to_string(d) + ": " + errs[d]); }
	for (size_t d = 0; d < K; ++d) { D.n_rec += n_rec[d]; D.computed.flags |= dig[d].flags; D.computed.add(0, dig[d].d[0]); D.computed.add(1, dig[d].d[1]); D.computed.add(3, dig[d].d[3]); }
	if (want_digest) { D.computed.flags |= 4u; D.computed.add(2, hc.digest); }
	D.domains = K; D.at_a_time = T;
	if (!writing) return true;
	FILE* out = fopen(out_path.c_str(), "wb");
	if (!out) die("cannot open file: " + out_path);
	std::vector<char> buf(1 << 24); bool ok = true;
	for (size_t d = 0; d < K && ok; ++d)
	{
		FILE* in = fopen(tmp[d].c_str(), "rb");
		if (!in) { ok = false; break; }
		for (size_t got; (got = fread(buf.data(), 1, buf.size(), in)) > 0; ) if (fwrite(buf.data(), 1, got, out) != got) { ok = false; break; }
		fclose(in); remove(tmp[d].c_str());
	}
	if (fflush(out) != 0 || ferror(out)) ok = false;
	if (fclose(out) != 0) ok = false;
	if (!ok) die("cannot write " + out_path + " (disk full?)");
	return true;
}

// The records of an archive in file order, written to out_path (empty: decoded only).  remove_on_error: a decoding error takes the
// output file with it (an archive whose content digest is being checked leaves no half-written or unconfirmed file behind).
// gpu >= 0 (`--gpu N`): the quality stream of an archive with `hipqdomains` is decoded on that device; any other archive on the host as ever
static void decode_archive(const std::string& arc, const std::string& genome, const std::string& out_path, int dom_threads, bool want_digest, bool want_values, bool remove_on_error, int gpu, Decoded& D)
{
	auto fail = [&](const std::string& m) { if (remove_on_error && !out_path.empty()) (void)remove(out_path.c_str()); die(m); };
	const char* why_host = "--gpu: the archive has no `hipqdomains` stream (it was written without --qual-domain-symbols): its quality stream is one dependent chain per domain and is decoded on the host";
	try { if (decode_domains(arc, genome, out_path, dom_threads, want_digest, want_values, D)) { if (gpu >= 0) fprintf(stderr, "colord_hip: %s\n", why_host); return; } } catch (const std::exception& e) { fail(e.what()); }
	bool write_ok = true;
	DeviceQualDecoder dev(gpu);                                                // (outlives the record stream, whose quality thread calls it)
	try
	{
		RecordStream rs(arc, genome);
		if (want_digest) rs.enable_digest();
		if (want_values) rs.enable_digest_values();
		if (D.want_report) rs.enable_report();
		if (gpu >= 0)
		{
			if (rs.n_qual_domains())
			{
				uint64_t max_bases = 1ull << 30;
				if (const char* e = getenv("COLORD_HIP_QDEC_BATCH_BASES")) max_bases = strtoull(e, nullptr, 10);
				rs.set_qual_batch_decoder(std::ref(dev), max_bases);
			}
			else fprintf(stderr, "colord_hip: %s\n", why_host);
		}
		FILE* out = out_path.empty() ? nullptr : fopen(out_path.c_str(), "wb");
		if (!out_path.empty() && !out) die("cannot open file: " + out_path);
		std::vector<char> obuf(out ? 1 << 24 : 1); if (out) setvbuf(out, obuf.data(), _IOFBF, obuf.size());
		const bool is_fastq = rs.is_fastq();
		// writer (decompression.cpp:84-258): records in file order; the three streams are packed independently
		std::vector<char> line; Record r;
		try
		{
			while (rs.next(r))
			{
				if (out) { format_record(line, r, is_fastq); if (fwrite(line.data(), 1, line.size(), out) != line.size()) { write_ok = false; break; } }
				++D.n_rec;
			}
		}
		catch (...) { if (out) fclose(out); throw; }
		if (out && (fflush(out) != 0 || ferror(out))) write_ok = false;
		if (out && fclose(out) != 0) write_ok = false;
		if (want_digest && write_ok) D.computed = rs.digests();
		if (D.want_report && write_ok) rs.report_into(D.report, D.lens);
		dev.report();
	}
	catch (const std::exception& e) { fail(e.what()); }
	if (!write_ok) fail("cannot write " + out_path + " (disk full?)");
}

int run_decompress(int argc, char** argv)
{
	std::vector<std::string> pos; std::string genome; int dom_threads = (int)std::min<unsigned>(16, std::max<unsigned>(1, std::thread::hardware_concurrency() / 3));
	bool ignore_digest = false; int gpu = -1;
	for (int i = 2; i < argc; ++i)
	{
		const std::string a = argv[i];
		if ((a == "-G" || a == "--reference-genome") && i + 1 < argc) genome = argv[++i];      // needed when the archive was written with -G but without -s
		else if (a == "--gpu" && i + 1 < argc) gpu = gpu_number(argv[++i]);
		else if (a == "-v" || a == "--verbose") ;
		else if ((a == "-t" || a == "--threads") && i + 1 < argc) dom_threads = atoi(argv[++i]);
		else if (a == "--ignore-digest") ignore_digest = true;                                  // salvage: decode whatever the stored content digest says
		else pos.push_back(a);
	}
	if (pos.size() != 2) { fprintf(stderr, "usage: colord_hip decompress [-G reference_genome.fa] [--ignore-digest] [--gpu N] archive.colord output.fastq\n"); return 1; }
	// an archive written with --digest is checked while it is decoded: the stream threads digest what they decode
	DigestSet stored; const int have = ignore_digest ? 0 : read_hipdigest(pos[0], stored);
	if (have < 0) die("the archive's `hipdigest` stream is not one this build reads (--ignore-digest decodes without the check)");
	// ... and one written with --report likewise: the output side of the stored content report against what is decoded
	ReportSet stored_rep; const int have_rep = ignore_digest ? 0 : read_hipreport(pos[0], stored_rep);
	if (have_rep < 0) die("the archive's `hipreport` stream is not one this build reads (--ignore-digest decodes without the check)");
	Decoded D; D.want_report = have_rep > 0;
	// (the qual-values digest only where the archive stores one: --digest-values)
	decode_archive(pos[0], genome, pos[1], dom_threads, have > 0, have > 0 && ((stored.flags >> 3) & 1), have > 0 || have_rep > 0, gpu, D);
	if (have > 0)
	{
		const std::string bad = digest_mismatch(stored, D.computed);
		if (!bad.empty()) { (void)remove(pos[1].c_str()); die("content digest mismatch, the archive does not hold what was compressed: " + bad + " (no output was written; --ignore-digest decodes regardless)"); }
		fprintf(stderr, "content digest: ok (%s)\n", stored.names().c_str());
	}
	if (have_rep > 0)
	{
		D.report.n50 = rp_nxx(D.lens, 50); D.report.n90 = rp_nxx(D.lens, 90);
		const std::string bad = report_mismatch(stored_rep, D.report);
		if (!bad.empty()) { (void)remove(pos[1].c_str()); die("content report mismatch, the archive does not hold what was compressed: " + bad + " (no output was written; --ignore-digest decodes regardless)"); }
		fprintf(stderr, "content report: ok\n");
	}
	if (D.domains) fprintf(stderr, "colord_hip: %llu records decompressed (%zu independent domains, %zu at a time)\n", (unsigned long long)D.n_rec, D.domains, D.at_a_time);
	else fprintf(stderr, "colord_hip: %llu records decompressed\n", (unsigned long long)D.n_rec);
	return 0;
}

// `colord_hip check archive.colord [-G genome]`: decodes everything, writes nothing; the content digests of what was decoded, the stored
// ones where the archive has them (also archives of the reference, which have none), exit 1 where they differ or the archive does not decode
int run_check(int argc, char** argv)
{
	std::vector<std::string> pos; std::string genome; int dom_threads = (int)std::min<unsigned>(16, std::max<unsigned>(1, std::thread::hardware_concurrency() / 3));
	int gpu = -1;
	for (int i = 2; i < argc; ++i)
	{
		const std::string a = argv[i];
		if ((a == "-G" || a == "--reference-genome") && i + 1 < argc) genome = argv[++i];
		else if (a == "--gpu" && i + 1 < argc) gpu = gpu_number(argv[++i]);
		else if ((a == "-t" || a == "--threads") && i + 1 < argc) dom_threads = atoi(argv[++i]);
		else pos.push_back(a);
	}
	if (pos.size() != 1) { fprintf(stderr, "usage: colord_hip check [-G reference_genome.fa] [--gpu N] archive.colord\n"); return 1; }
	DigestSet stored; const int have = read_hipdigest(pos[0], stored);
	ReportSet stored_rep; const int have_rep = read_hipreport(pos[0], stored_rep);
	Decoded D; D.want_report = true;
	decode_archive(pos[0], genome, "", dom_threads, true, true, false, gpu, D);
	D.report.n50 = rp_nxx(D.lens, 50); D.report.n90 = rp_nxx(D.lens, 90);
	// the content report: without a stored one the output side of what was decoded is printed; with one the two are compared
	int rep_status = 0;
	auto check_report = [&]() {
		if (have_rep == 0) { printf("decoded content (no content report is stored in this archive; written without --report):\n"); print_report(stdout, D.report, true); return; }
		if (have_rep < 0) { printf("the archive's `hipreport` stream is not one this build reads\n"); rep_status = 1; return; }
		const std::string bad = report_mismatch(stored_rep, D.report);
		if (!bad.empty()) { printf("content report mismatch: %s\n", bad.c_str()); rep_status = 1; return; }
		printf("content report: ok\n");
	};
	for (int i = 0; i < 3; ++i) printf("%s\n", D.computed.line(i).c_str());
	if ((D.computed.flags >> 3) & 1) printf("%s\n", D.computed.line(3).c_str());      // (any archive with a coded quality stream, the reference's included)
	check_report();
	if (have == 0) { printf("no content digest is stored in this archive (written without --digest); %llu records decode\n", (unsigned long long)D.n_rec); return rep_status; }
	if (have < 0) { printf("the archive's `hipdigest` stream is not one this build reads\n"); return 1; }
	for (int j = 0; j < 4; ++j) if (const int i = DigestSet::in_order(j); (stored.flags >> i) & 1) printf("stored %s\n", stored.line(i).c_str());
	const std::string bad = digest_mismatch(stored, D.computed);
	if (!bad.empty()) { printf("content digest mismatch: %s\n", bad.c_str()); return 1; }
	printf("content digest: ok (%s)\n", stored.names().c_str());
	return rep_status;
}
