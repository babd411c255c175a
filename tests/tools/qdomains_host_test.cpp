// qdomains_host_test.cpp — the host code behind the model domains of the quality stream as a stand-alone program (own main, nothing
// preloaded), for a build under AddressSanitizer and UBSan (tests/test_qual_domains_cpu.py builds and runs it): the `hipqdomains` parser
// and the batching of whole domains in cli/reader.hpp, over the library's decoders compiled for the host into this program.
//   qdomains_host_test ARCHIVE [MAX_BASES]
// decodes the archive twice through RecordStream — part by part with fresh models at every domain start, and in batches of whole domains
// of at most MAX_BASES bases (default 50000: several batches) handed to a batch decoder that runs the host decoder — and compares the
// two record by record.  A corrupt archive is a message ("error: ...") and exit 3: an exception, never a read out of range.
#include "../../colord_amd/csrc/decode.hip"
#include "../../colord_amd/csrc/genome.hip"
#include "../../colord_amd/csrc/cli/reader.hpp"
#include <cinttypes>

using namespace colord_hip_reader;

struct Rec { std::string id, bases, quals; };

// the batch decoder of the test: the host decoder over the batch's parts, fresh models at every domain start
struct HostBatches {
	uint64_t batches = 0, domains = 0;
	void operator()(const cl_qual_params& qp, QualBatch& B, cl_digest* acc)
	{
		cl_qual_decoder* q = nullptr;
		if (cl_qual_decoder_create(&qp, &q) != CL_OK) throw std::runtime_error("cl_qual_decoder_create");
		if (acc && cl_qual_decoder_set_digest(q, 1, B.first_read) != CL_OK) { cl_qual_decoder_free(q); throw std::runtime_error("cl_qual_decoder_set_digest"); }
		if (B.domain_first.empty() || B.domain_first[0] != 0 || B.payloads.size() != B.parts.size()) { cl_qual_decoder_free(q); throw std::runtime_error("a batch starts with a domain"); }
		size_t d = 1; uint64_t reads = 0, bases = 0;
		for (size_t p = 0; p < B.parts.size(); ++p)
		{
			if (d < B.domain_first.size() && B.domain_first[d] == p) { cl_qual_decoder_new_domain(q); ++d; }
			ReadPart& x = B.parts[p];
			x.quals.resize(x.bases.size());
			if (cl_qual_decode_part(q, B.payloads[p].data(), B.payloads[p].size(), x.bases.data(), x.off.data(), (uint32_t)(x.off.size() - 1), x.quals.data()) != CL_OK) { cl_qual_decoder_free(q); throw std::runtime_error("corrupt `qual` part"); }
			reads += x.off.size() - 1; bases += x.bases.size();
		}
		if (d != B.domain_first.size() || reads != B.n_reads || bases != B.n_bases) { cl_qual_decoder_free(q); throw std::runtime_error("the batch's counts do not fit its parts"); }
		if (acc) { cl_digest g{ 0, 0, 0 }; cl_qual_decoder_digest(q, &g); acc->reads += g.reads; acc->symbols += g.symbols; acc->sum += g.sum; }
		cl_qual_decoder_free(q);
		++batches; domains += B.domain_first.size();
	}
};

static DigestSet decode(const char* path, HostBatches* hb, uint64_t max_bases, std::vector<Rec>& out, size_t& n_domains)
{
	RecordStream rs(path);
	rs.enable_digest();
	n_domains = rs.n_qual_domains();
	if (hb) rs.set_qual_batch_decoder(std::ref(*hb), max_bases);
	Record r;
	while (rs.next(r)) out.push_back(Rec{ std::string((const char*)r.header, r.header_len), std::string((const char*)r.bases, r.n_bases), r.quals ? std::string((const char*)r.quals, r.n_bases) : std::string() });
	return rs.digests();
}

int main(int argc, char** argv)
{
	if (argc < 2) { fprintf(stderr, "usage: qdomains_host_test ARCHIVE [MAX_BASES]\n"); return 2; }
	const uint64_t max_bases = argc > 2 ? strtoull(argv[2], nullptr, 10) : 50000;
	try
	{
		std::vector<Rec> a, b; size_t nd = 0; HostBatches hb;
		const DigestSet da = decode(argv[1], nullptr, 0, a, nd);
		const DigestSet db = decode(argv[1], &hb, max_bases, b, nd);
		if (a.size() != b.size()) { printf("records differ: %zu, %zu\n", a.size(), b.size()); return 1; }
		for (size_t i = 0; i < a.size(); ++i) if (a[i].id != b[i].id || a[i].bases != b[i].bases || a[i].quals != b[i].quals) { printf("record %zu differs\n", i); return 1; }
		if (!digest_mismatch(da, db).empty() || da.flags != db.flags) { printf("digests differ: %s\n", digest_mismatch(da, db).c_str()); return 1; }
		for (int i = 0; i < 3; ++i) printf("%s\n", da.line(i).c_str());
		for (const Rec& r : a) { for (char c : r.bases) putchar("ACGTN"[(c & 7) > 4 ? 4 : (c & 7)]); putchar('\t'); fputs(r.quals.c_str(), stdout); putchar('\n'); }
		printf("ok: %zu records, %zu domains, %" PRIu64 " batches of %" PRIu64 " domains\n", a.size(), nd, hb.batches, hb.domains);
		return 0;
	}
	catch (const std::exception& e) { printf("error: %s\n", e.what()); return 3; }
}
