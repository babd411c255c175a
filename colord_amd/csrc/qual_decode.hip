// qual_decode.hip — the quality stream DECODED on the device (CQualityCoder::Decode, quality_coder.cpp:605-657, quality_coder_impl.cpp
// decode_* incl. :506-559, :800-849; driver CEntrDecomprQuals, entr_qual.h:136-260; CRangeDecoder, sub_rc.h:216-392).
//
// In a decoder the symbol just decoded selects the next context and updates the model the next symbol may need: one model domain is ONE
// dependent chain, and the reference's file is one domain.  An archive written with model domains (cl_qual_coder_set_domain_symbols)
// holds many: every domain starts from the initial models and is a whole number of parts, so the domains decode side by side — ONE LANE
// PER DOMAIN here, each with model tables of its own in HBM, the interval coder restarting per part as in the host decoder.  A lane's
// chain is latency bound (every symbol: model row load -> search -> interval step -> model store); the launch wins by the number of
// domains in flight only.  The first kernel of this library that evolves models from decoded symbols instead of checking intervals.
//
// What is shared, not restated: the interval step is rc_check_step / rc_quotient (rc_check.hpp), the byte window RcDevBytes; the context
// of a position is qual_hist_of / qual_base_ctx_at / qual_ctx_id (qual_ctx.hpp), the very functions k_qual_symbols codes with.
//
// Bounds by construction (the input may be anything):
//   * every loop bound is known before the loop starts: parts of a domain, reads of a part, bases of a read (the arena's lengths),
//     the alphabet; a part decodes exactly the symbols its reads' lengths ask for;
//   * payload bytes are read through RcDevBytes, clamped to [0, size) of the part, which lies inside d_in (checked on the host); bytes
//     past the end read as 0, as the host decoder reads them;
//   * a context id is below n_ctx and a symbol below n_sym whatever was decoded (fields, base codes and flags are bounded by their
//     own construction); a total stays below max_total <= 2^20 < the reciprocal table's 2^21 entries: the tables are the kernel's own;
//   * the output offsets are checked against the arena's lengths and the buffers' capacities before the launch (k_qdec_offsets).
// A part whose symbols leave their intervals or that does not end at its size stops its domain: the lane writes the part and goes idle.
#include "common.hpp"
#include "objects.hpp"
#include "rc_dev.hpp"
#include "rc_check.hpp"
#include "qual_ctx.hpp"
#include <string>
#include <vector>

namespace {

struct QualDecRev { uint8_t v[8]; };                       // the -D representatives of the bins (none: v[0])
enum : uint32_t { QDEC_OK = 0, QDEC_SYMBOL = 1, QDEC_END = 2, QDEC_SIZE = 3 };

// d_qual_off against the arena: read r has lens[r] bytes at qual_off[r], the offsets ascend and end inside the buffers
__global__ void k_qdec_offsets(const uint64_t* __restrict__ qoff, const uint32_t* __restrict__ lens, uint32_t n_reads, uint64_t quals_cap, uint32_t* __restrict__ bad)
{
	const uint64_t r = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
	if (r >= n_reads) return;
	const uint64_t a = qoff[r], b = qoff[r + 1];
	if (b < a || b - a != lens[r] || b > quals_cap) atomicOr(bad, 1u);
}

// the lane's models: rows of n_sym counters and their total
struct QDecModels {
	uint32_t* tab; uint32_t n_sym, max_total, adder;
	const uint64_t* __restrict__ inv_tab;
	// One symbol from the model of context c: found by comparing q t <= buffer for the cumulative counts t (GetCumulativeFreq without its
	// second division, as host_coder.hpp), taken through rc_check_step (which refuses a buffer outside the symbol's interval: a corrupt
	// part), then +adder and halve-round-up at max_total (rc.h:233-244).  false: the part does not decode; nothing is updated then.
	template<class Src>
	__device__ inline bool decode(uint64_t c, uint64_t& low, uint64_t& range, uint64_t& buffer, Src& src, uint32_t& sym_out)
	{
		uint32_t* m = tab + c * (n_sym + 1);
		const uint32_t tot = m[n_sym];
		const uint64_t inv = inv_tab[tot & (INV_TABLE_SIZE - 1)];
		const uint64_t q = tot ? rc_quotient(range, tot, inv) : 0;
		uint32_t cum = 0, freq = 0, sym = n_sym - 1; bool found = false;
		for (uint32_t i0 = 0; i0 < n_sym && !found; i0 += 8)                     // (eight independent loads a round)
		{
			uint32_t v[8];
#pragma unroll
			for (uint32_t u = 0; u < 8; ++u) v[u] = i0 + u < n_sym ? m[i0 + u] : 0u;
#pragma unroll
			for (uint32_t u = 0; u < 8; ++u)
				if (!found && i0 + u < n_sym)
				{
					const uint64_t nt = (uint64_t)cum + v[u];
					if (nt * q > buffer || i0 + u + 1 == n_sym) { sym = i0 + u; freq = v[u]; found = true; }   // (the last symbol takes what lies beyond: the step judges it)
					else cum = (uint32_t)nt;
				}
		}
		const uint64_t t = ((uint64_t)cum << 42) | ((uint64_t)freq << 21) | tot;
		if (tot >= INV_TABLE_SIZE || !rc_check_step(low, range, buffer, t, inv, src)) return false;
		m[sym] = freq + adder;
		uint32_t nt = tot + adder;
		for (uint32_t round = 0; round < 32 && nt >= max_total; ++round)          // (one round nearly always: a round halves what exceeds n_sym)
		{
			nt = 0;
			for (uint32_t a = 0; a < n_sym; ++a) { const uint32_t v = (m[a] + 1) / 2; m[a] = v; nt += v; }
		}
		m[n_sym] = nt;
		sym_out = sym;
		return true;
	}
};

// One lane per domain, one wave per 64 domains of the launch.  Domain d = d0 + slot decodes the parts [dom_first[d], dom_first[d + 1]);
// its tables are slot `slot` of state / bstate.  status[2 slot] = QDEC_* << 32 | the part that failed, status[2 slot + 1] = the bytes
// that part's decoder asked for.
__global__ __launch_bounds__(64) void k_qual_decode(const QualCfg* __restrict__ cfgp, QualDecRev rev,
                                                   const uint64_t* __restrict__ packed, const uint64_t* __restrict__ word_off, const uint32_t* __restrict__ lens,
                                                   const uint8_t* __restrict__ flags, const uint64_t* __restrict__ qoff,
                                                   const uint8_t* __restrict__ in, const uint64_t* __restrict__ part_off, const uint64_t* __restrict__ part_size,
                                                   const uint32_t* __restrict__ part_bounds, const uint32_t* __restrict__ dom_first, uint32_t d0, uint32_t nd,
                                                   uint32_t* __restrict__ state, uint64_t state_words, uint32_t* __restrict__ bstate, const uint64_t* __restrict__ inv_tab,
                                                   uint8_t* __restrict__ quals, uint8_t* __restrict__ symbols, uint64_t* __restrict__ status)
{
	__shared__ QualCfg cfg;
	__shared__ double s_avg[5][64], s_as[5][64], s_qs[5][64];                  // *-avg: a lane's averages and error-diffusion sums, [bin][lane]
	for (uint32_t i = threadIdx.x; i < sizeof(QualCfg) / 4; i += blockDim.x) ((uint32_t*)&cfg)[i] = ((const uint32_t*)cfgp)[i];
	__syncthreads();
	const uint32_t lane = threadIdx.x, slot = blockIdx.x * 64 + lane;
	if (slot >= nd) return;
	const uint32_t d = d0 + slot;
	const int32_t mode = cfg.mode;
	const uint32_t navg = cfg.navg, n_bins = cfg.n_bins;
	const bool per_base = mode <= QM_BINARY_THR;
	QDecModels sym_m{ state + (uint64_t)slot * state_words, cfg.n_sym, cfg.max_total, cfg.adder, inv_tab };
	QDecModels byte_m{ bstate + (uint64_t)slot * ((uint64_t)QUAL_BYTE_CTX * 257), 256u, QUAL_BYTE_MAX_TOTAL, QUAL_BYTE_ADDER, inv_tab };
	uint32_t fail = QDEC_OK, fail_part = 0; uint64_t fail_bytes = 0;
	const uint32_t pa = dom_first[d], pe = dom_first[d + 1];
	for (uint32_t p = pa; p < pe && fail == QDEC_OK; ++p)
	{
		const uint32_t ra = part_bounds[p], re = part_bounds[p + 1];
		if (mode == QM_NONE)
		{	// nothing is coded: the representative of the only bin (quality_coder.cpp:611-617)
			for (uint32_t r = ra; r < re; ++r) { const uint64_t qb = qoff[r]; const uint32_t len = lens[r]; for (uint32_t i = 0; i < len; ++i) quals[qb + i] = (uint8_t)(33 + rev.v[0]); }
			continue;
		}
		const uint64_t size = part_size[p];
		if (size < 8) { fail = QDEC_SIZE; fail_part = p; break; }
		RcDevBytes src; src.start(in + part_off[p], size);
		uint64_t low = 0, range = RC_MASK, buffer = src.peek8();
		src.advance(8);
		bool ok = true;
		for (uint32_t r = ra; r < re && ok; ++r)
		{
			const uint64_t qb = qoff[r], wb = word_off[r]; const uint32_t len = lens[r];
			uint8_t* so = symbols ? symbols + (uint64_t)r * navg + (per_base ? qb : 0) : nullptr;
			// the average bytes in front of the read's symbols (quality_coder_impl.cpp:821-849)
			auto dec_avg = [&](uint32_t bin, uint32_t ctx_p, uint32_t k, double& avg) -> bool {
				uint32_t a1 = 0, a2 = 0;
				if (!byte_m.decode(qual_avg_ctx_hi(bin, ctx_p), low, range, buffer, src, a1)) return false;
				if (!byte_m.decode(qual_avg_ctx_lo(a1), low, range, buffer, src, a2)) return false;
				if (so) { so[2 * k] = (uint8_t)a1; so[2 * k + 1] = (uint8_t)a2; }
				avg = (double)((a1 << 8) + a2) / 256.0;
				return true;
			};
			if (mode == QM_AVERAGE)
			{	// decode_average (:800-817)
				double avg = 0.0, as = 0.0, qs = 0.0;
				ok = dec_avg(0, 0, 0, avg);
				if (ok) for (uint32_t i = 0; i < len; ++i) { as += avg; const uint32_t v = (uint32_t)(as - qs); qs += v; quals[qb + i] = (uint8_t)(v + 33); }
				continue;
			}
			if (cfg.is_avg)
			{
				uint32_t ctx_p = 0;
				for (uint32_t t = 0; t < n_bins && ok; ++t)
				{
					double avg = 0.0;
					ok = dec_avg(t, ctx_p, t, avg);
					s_avg[t][lane] = avg; s_as[t][lane] = 0.0; s_qs[t][lane] = 0.0;
					ctx_p = (uint32_t)avg;
				}
			}
			uint64_t ring = 0;                                                      // the history fields of the positions before, the last one lowest, 8 bits each (n_ctx_sym <= 6)
			for (uint32_t i = 0; i < len && ok; ++i)
			{
				const uint32_t hist = qual_hist_of(cfg, i, [&](uint32_t t) { return (uint32_t)(ring >> (8 * (t - 1))) & 0xffu; });
				const uint32_t bctx = qual_base_ctx_at(cfg, packed, wb, i, len);
				const uint32_t fl = cfg.level > 1 && flags ? qual_flag_bits(flags[qb + i]) : 0u;
				uint32_t s = 0;
				ok = sym_m.decode(qual_ctx_id(cfg, hist, bctx, fl), low, range, buffer, src, s);
				if (!ok) break;
				if (so) so[navg + i] = (uint8_t)s;
				uint32_t v;
				if (cfg.is_avg)
				{	// error diffusion in IEEE double (:506-559)
					const double as = s_as[s][lane] + s_avg[s][lane];
					const double qs = s_qs[s][lane];
					v = (uint32_t)(as - qs);
					s_as[s][lane] = as; s_qs[s][lane] = qs + v;
				}
				else v = mode == QM_ORIGINAL ? s : rev.v[s & 7];
				quals[qb + i] = (uint8_t)(v + 33);
				ring = (ring << 8) | qual_hist_field(cfg, s);
			}
		}
		if (!ok) { fail = QDEC_SYMBOL; fail_part = p; fail_bytes = src.pos; }
		else if (src.pos != size) { fail = QDEC_END; fail_part = p; fail_bytes = src.pos; }
	}
	status[2 * (uint64_t)slot] = ((uint64_t)fail << 32) | fail_part;
	status[2 * (uint64_t)slot + 1] = fail_bytes;
}

} // namespace

// CEntrDecomprQuals (entr_qual.h:136-260) over CQualityCoder::Decode (quality_coder.cpp:605-657, quality_coder_impl.cpp:506-559,800-849)
// and CRangeDecoder (sub_rc.h:216-392), for the model domains of an archive written with cl_qual_coder_set_domain_symbols.
extern "C" cl_status cl_qual_decode_domains(cl_ctx* ctx, const cl_qual_params* qparams, const cl_reads* R, const uint8_t* d_flags,
                                            const uint8_t* d_in, uint64_t n_in, const uint32_t* h_part_bounds, const uint64_t* h_part_sizes, uint32_t n_parts,
                                            const uint32_t* h_domain_first_part, uint32_t n_domains, uint32_t max_domains_per_launch,
                                            uint8_t* d_quals, const uint64_t* d_qual_off, uint64_t quals_cap, uint8_t* d_symbols, uint64_t symbols_cap)
{
	if (!ctx || !qparams || !R || !h_part_bounds || !h_part_sizes || !h_domain_first_part || !d_qual_off) return cl_fail(ctx, CL_E_INVALID, "cl_qual_decode_domains: null argument");
	if (!n_parts || !n_domains) return (n_parts || n_domains) ? cl_fail(ctx, CL_E_INVALID, "cl_qual_decode_domains: parts without domains or domains without parts") : CL_OK;
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	QualCfg c;
	{	// (an archive's `meta` stream carries no -T thresholds: a decoder never maps a quality to its bin.  The configuration asks for
		// them all the same — they fill map_fwd, which nothing here reads — so a caller may leave them out)
		cl_qual_params prm = *qparams;
		static const uint32_t bins_of[9] = { 0, 5, 4, 2, 5, 4, 2, 0, 0 };
		if (prm.mode >= 0 && prm.mode <= 8 && bins_of[prm.mode] && prm.n_fwd == 0) { prm.n_fwd = bins_of[prm.mode] - 1; for (uint32_t i = 0; i < prm.n_fwd; ++i) prm.fwd[i] = i + 1; }
		CL_TRY(qual_make_cfg(ctx, &prm, c));
	}
	if (qparams->n_rev > 8) return cl_fail(ctx, CL_E_INVALID, "cl_qual_decode_domains: more than 8 representatives");
	if (c.level > 1 && c.mode <= QM_BINARY_THR && !d_flags) return cl_fail(ctx, CL_E_INVALID, "cl_qual_decode_domains: levels 2 and 3 need the flags");
	QualDecRev rev{}; for (uint32_t i = 0; i < qparams->n_rev; ++i) rev.v[i] = (uint8_t)qparams->rev[i];
	// the shape of the call: ascending part bounds inside the arena, domains of at least one part that cover the parts, payloads inside d_in
	for (uint32_t p = 0; p < n_parts; ++p) if (h_part_bounds[p] > h_part_bounds[p + 1]) return cl_fail(ctx, CL_E_INVALID, "cl_qual_decode_domains: part bounds must ascend");
	if (h_part_bounds[n_parts] > R->n_reads) return cl_fail(ctx, CL_E_INVALID, "cl_qual_decode_domains: part bound beyond the arena");
	if (h_domain_first_part[0] != 0) return cl_fail(ctx, CL_E_INVALID, "cl_qual_decode_domains: the first domain starts at part 0");
	for (uint32_t d = 0; d < n_domains; ++d)
		if (h_domain_first_part[d] >= n_parts || (d && h_domain_first_part[d] <= h_domain_first_part[d - 1])) return cl_fail(ctx, CL_E_INVALID, "cl_qual_decode_domains: domain starts must ascend and lie inside the parts");
	std::vector<uint64_t> part_off(n_parts + 1); part_off[0] = 0;
	for (uint32_t p = 0; p < n_parts; ++p)
	{
		if (h_part_sizes[p] > n_in - part_off[p]) return cl_fail(ctx, CL_E_INVALID, "cl_qual_decode_domains: the parts' sizes exceed the input");
		part_off[p + 1] = part_off[p] + h_part_sizes[p];
	}
	if (c.mode != QM_NONE && !d_in) return cl_fail(ctx, CL_E_INVALID, "cl_qual_decode_domains: null argument");
	const uint32_t n_reads = R->n_reads;
	if (R->total_bases && !d_quals) return cl_fail(ctx, CL_E_INVALID, "cl_qual_decode_domains: null argument");
	const bool per_base = c.mode <= QM_BINARY_THR;
	// the outputs: read r at d_qual_off[r], as long as the arena says
	{
		DevBuf<uint32_t> bad; DEV_ALLOC(ctx, bad, 1);
		HIP_TRY(ctx, hipMemsetAsync(bad.p, 0, 4, ctx->stream));
		if (n_reads) LAUNCH(ctx, k_qdec_offsets, grid_for(n_reads, 256), 256, d_qual_off, (const uint32_t*)R->lens.p, n_reads, quals_cap, bad.p);
		HIP_TRY(ctx, hipGetLastError());
		uint32_t h_bad = 0; uint64_t q_end = 0;
		HIP_TRY(ctx, hipMemcpyAsync(&h_bad, bad.p, 4, hipMemcpyDeviceToHost, ctx->stream));
		HIP_TRY(ctx, hipMemcpyAsync(&q_end, d_qual_off + n_reads, 8, hipMemcpyDeviceToHost, ctx->stream));
		HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
		if (h_bad) return cl_fail(ctx, CL_E_INVALID, "cl_qual_decode_domains: d_qual_off does not hold the arena's read lengths inside quals_cap");
		if (d_symbols && c.mode != QM_NONE && (uint64_t)n_reads * c.navg + (per_base ? q_end : 0) > symbols_cap) return cl_fail(ctx, CL_E_CAPACITY, "cl_qual_decode_domains: symbols_cap");
	}
	// domains per launch: what the budget holds of their model tables (COLORD_HIP_QDEC_BUDGET_MB, default 4096 MB; one domain always)
	const uint64_t state_words = (uint64_t)c.n_ctx * (c.n_sym + 1), bstate_words = (uint64_t)QUAL_BYTE_CTX * 257;
	uint64_t budget = 4096ull << 20;
	if (const char* e = getenv("COLORD_HIP_QDEC_BUDGET_MB")) budget = (uint64_t)std::max(1, atoi(e)) << 20;
	uint64_t batch = std::max<uint64_t>(1, budget / ((state_words + bstate_words) * 4));
	if (max_domains_per_launch) batch = std::min<uint64_t>(batch, max_domains_per_launch);
	batch = std::min<uint64_t>(batch, n_domains);
	const uint64_t* inv_tab = nullptr;
	CL_TRY(cl_inv_table(ctx, &inv_tab));
	DevBuf<QualCfg> d_cfg; DevBuf<uint64_t> d_part_off, d_part_size, d_status; DevBuf<uint32_t> d_pb, d_dom, state, bstate;
	std::vector<uint32_t> dom(h_domain_first_part, h_domain_first_part + n_domains); dom.push_back(n_parts);
	DEV_ALLOC(ctx, d_cfg, 1); DEV_ALLOC(ctx, d_part_off, (uint64_t)n_parts + 1); DEV_ALLOC(ctx, d_part_size, n_parts); DEV_ALLOC(ctx, d_pb, (uint64_t)n_parts + 1);
	DEV_ALLOC(ctx, d_dom, (uint64_t)n_domains + 1); DEV_ALLOC(ctx, d_status, 2 * batch);
	DEV_ALLOC(ctx, state, batch * state_words); DEV_ALLOC(ctx, bstate, batch * bstate_words);
	HIP_TRY(ctx, hipMemcpyAsync(d_cfg.p, &c, sizeof(c), hipMemcpyHostToDevice, ctx->stream));
	HIP_TRY(ctx, hipMemcpyAsync(d_part_off.p, part_off.data(), ((uint64_t)n_parts + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
	HIP_TRY(ctx, hipMemcpyAsync(d_part_size.p, h_part_sizes, (uint64_t)n_parts * 8, hipMemcpyHostToDevice, ctx->stream));
	HIP_TRY(ctx, hipMemcpyAsync(d_pb.p, h_part_bounds, ((uint64_t)n_parts + 1) * 4, hipMemcpyHostToDevice, ctx->stream));
	HIP_TRY(ctx, hipMemcpyAsync(d_dom.p, dom.data(), ((uint64_t)n_domains + 1) * 4, hipMemcpyHostToDevice, ctx->stream));
	std::vector<uint64_t> st(2 * batch);
	std::string first_bad;
	for (uint64_t d0 = 0; d0 < n_domains; d0 += batch)
	{
		const uint32_t nd = (uint32_t)std::min<uint64_t>(batch, n_domains - d0);
		if (c.mode != QM_NONE)
		{
			CL_TRY(qual_init_state(ctx, state.p, (uint64_t)nd * c.n_ctx, c.n_sym));
			if (c.navg) CL_TRY(qual_init_state(ctx, bstate.p, (uint64_t)nd * QUAL_BYTE_CTX, 256u));
		}
		LAUNCHB(ctx, 0.0, k_qual_decode, grid_for(nd, 64), 64, (const QualCfg*)d_cfg.p, rev, (const uint64_t*)R->packed.p, (const uint64_t*)R->word_off.p, (const uint32_t*)R->lens.p,
			d_flags, d_qual_off, d_in, (const uint64_t*)d_part_off.p, (const uint64_t*)d_part_size.p, (const uint32_t*)d_pb.p, (const uint32_t*)d_dom.p, (uint32_t)d0, nd,
			state.p, state_words, bstate.p, inv_tab, d_quals, c.mode == QM_NONE ? nullptr : d_symbols, d_status.p);
		HIP_TRY(ctx, hipGetLastError());
		HIP_TRY(ctx, hipMemcpyAsync(st.data(), d_status.p, 2ull * nd * 8, hipMemcpyDeviceToHost, ctx->stream));
		HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
		for (uint32_t s = 0; s < nd && first_bad.empty(); ++s)
		{
			const uint32_t kind = (uint32_t)(st[2 * s] >> 32), part = (uint32_t)st[2 * s];
			if (kind == QDEC_OK) continue;
			first_bad = "coded qual stream: domain " + std::to_string(d0 + s) + ", part " + std::to_string(part) + " (" + std::to_string(h_part_sizes[part]) + " bytes) ";
			if (kind == QDEC_SIZE) first_bad += "has fewer than the 8 bytes every part has";
			else if (kind == QDEC_SYMBOL) first_bad += "does not decode: a symbol lies outside its model's interval after " + std::to_string(st[2 * s + 1]) + " bytes";
			else first_bad += "does not end at its size: the decoder consumes " + std::to_string(st[2 * s + 1]) + " bytes";
		}
	}
	cl_timing_collect(ctx);
	// (every domain was decoded: the qualities of the others are complete)
	if (!first_bad.empty()) return cl_fail(ctx, CL_E_MISMATCH, first_bad);
	return CL_OK;
}
