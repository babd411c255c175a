// expand.hip — the inverse of a10-a12 on the device: a read rebuilt from its own tuple stream and the reference reads it points to.
// What CEncoder::Encode (encoder.cpp:1672-1691) wrote is read back as CDNACoder::Decode (dna_coder.cpp:234-437) applies it, without
// the entropy coder in between: cl_es_expand stores the bases, cl_es_verify compares them with the arena the streams were made from.
//
// A read's tuples refer to reference reads only, so reads expand independently: ONE WAVE PER READ, walked as es_wave.hpp describes: the
// stream 64 bytes per window, the tuple starts from three ballots, the window cut into stretches that share a reference.  Here, within a
// stretch, two wave prefix sums (bases given, cursor advance) place every tuple; unit tuples store / compare their one base; anchors are
// copied by the whole wave, a base per lane straight from the packed words, in either orientation, whatever their alignment.
// So the time of a read grows with its stream bytes / 64 plus its anchor bases / 64, never with one lane's walk of the read.
//
// Bounds by construction (the kernel will meet the output of encoders that do not exist yet): those of es_wave.hpp, and: an anchor is
// checked against its reference's length and the read's measured length BEFORE its copy loop runs; every output index is checked
// against the measured length.  A malformed stream gives its read an error code (es_codes.hpp) and the call CL_E_INVALID.
#include "common.hpp"
#include "objects.hpp"
#include "es_wave.hpp"

namespace {
enum { EX_LEN = 0, EX_STORE = 1, EX_CMP = 2 };

// first_err / first_bad: read << 32 | (error code / first differing base, ~0 = none differs: length or tuple count), minimum over reads
struct ExResult { unsigned long long first_err, first_bad; unsigned int n_err, n_bad; };
__global__ void k_es_result_init(ExResult* res) { res->first_err = res->first_bad = ~0ull; res->n_err = res->n_bad = 0; }

// EX_LEN: out_len[r] = bases of read r.  EX_STORE: codes[base_off[r] ..] = its bases (0..4).  EX_CMP: compared with read r of `In`.
template<int MODE>
__global__ __launch_bounds__(64) void k_es_expand(Arena R, Arena In, const uint8_t* __restrict__ es, const uint64_t* __restrict__ es_off, const uint32_t* __restrict__ es_ntup,
                                                 uint32_t n_reads, uint32_t* __restrict__ out_len, uint8_t* __restrict__ codes, const uint64_t* __restrict__ base_off,
                                                 ExResult* __restrict__ res)
{
	const uint32_t r = blockIdx.x, lane = threadIdx.x;
	if (r >= n_reads) return;
	const uint64_t s0 = es_off[r], s1 = es_off[r + 1];
	const uint64_t n = s1 > s0 ? s1 - s0 : 0;                                   // stream bytes
	const uint8_t* s = es + s0;
	uint64_t L = 0, o0 = 0, in_wo = 0;                                          // measured length; where the bases go / come from
	if (MODE == EX_STORE) { o0 = base_off[r]; L = base_off[r + 1] - o0; }
	if (MODE == EX_CMP) { L = In.lens[r]; in_wo = In.word_off[r]; }
	uint32_t err = EDE_NONE;                                                    // uniform
	uint32_t lane_err = EDE_NONE, diff = 0xffffffffu;                           // per lane: what a base of mine ran into; first base of mine that differs
	uint64_t ocur = 0, tup = 0;                                                 // bases, tuples so far
	auto put = [&](uint64_t idx, uint32_t base) {
		if constexpr (MODE == EX_STORE) { if (idx < L) codes[o0 + idx] = (uint8_t)base; else lane_err = EDE_OUT_RANGE; }
		else if constexpr (MODE == EX_CMP)
		{	// (a base past the input's length: the lengths differ, seen at the end)
			if (idx < L)
			{
				const uint64_t w = in_wo + (idx >> 5); const uint32_t j = (uint32_t)idx & 31;
				const uint32_t have = (In.inv[w] >> (31 - j)) & 1u ? 4u : (uint32_t)(In.packed[w] >> (62 - 2 * j)) & 3u;
				if (have != base && (uint32_t)idx < diff) diff = (uint32_t)idx;
			}
		}
	};
	if (n == 0) err = EDE_EMPTY;
	else
	{
		const EsStart st = es_start(s, n, lane, R.n);
		if (st.plain)
		{	// the rest of the stream is `plain` tuples: a lane per base
			if (n - 1 > 0xffffffffull) err = EDE_TOO_LONG;
			else
			{
				for (uint64_t i = lane; i < n - 1; i += 64)
				{
					const uint32_t b = s[1 + i], e = es_plain_err(b);
					if (e) lane_err = e; else put(i, b & 0xf);
				}
				ocur = n - 1; tup = n;
			}
		}
		else if (st.err) err = st.err;
		else
		{
			EsRefs<true> F(R, st);
			uint64_t pos = 5; tup = 1;
			while (!err && pos < n)
			{
				const EsWindow W = es_window(s, pos, n, lane);
				if (W.err) { err = W.err; break; }
				const uint32_t t = W.t, outlen = es_read_adv(W), adv = es_ref_adv(W);
				const uint64_t sw = W.starts & (W.m5 | __ballot(t == T_MAIN_REF));   // tuples that change the reference
				const uint64_t anch = W.starts & __ballot(t == T_ANCHOR);
				uint64_t todo = W.starts;
				while (todo && !err)
				{	// a stretch of tuples on one reference, then the tuple that ends it
					const EsStretch x = es_stretch(todo, sw);
					if (x.seg)
					{
						const bool in_seg = (x.seg >> lane) & 1;
						const uint32_t ol = in_seg ? outlen : 0u, ad = in_seg ? adv : 0u;     // (at most 16 multi-byte tuples of 28 bits: the sums fit 32 bits)
						const uint32_t oi = wave_incl_scan(ol), ai = wave_incl_scan(ad);
						const uint32_t otot = __shfl(oi, 63, 64), atot = __shfl(ai, 63, 64);
						if (MODE != EX_LEN && in_seg)
						{
							const uint64_t my_o = ocur + (oi - ol), my_c = F.cursor + (ai - ad);
							const uint32_t v = W.b & 0xf;
							if (t == T_INS) { if (v > 3) lane_err = EDE_VALUE; else put(my_o, v); }
							else if (t == T_MATCH) { const uint32_t rb = ref_base(R, F.cur, my_c); if (rb > 3) lane_err = EDE_GUARD; else put(my_o, rb); }
							else if (t == T_SUBST)
							{	// v-th of the three bases other than the reference's
								const uint32_t rb = ref_base(R, F.cur, my_c);
								if (rb > 3) lane_err = EDE_GUARD; else if (v > 2) lane_err = EDE_VALUE; else put(my_o, v + (v >= rb ? 1u : 0u));
							}
						}
						for (uint64_t am = x.seg & anch; am; am &= am - 1)
						{	// an anchor: the whole wave copies it
							const uint32_t l = (uint32_t)__builtin_ctzll(am);
							const uint32_t alen = __shfl(W.v28, l, 64);
							const uint64_t a_c = F.cursor + (__shfl(ai, l, 64) - alen), a_o = ocur + (__shfl(oi, l, 64) - alen);
							if (a_c + alen > F.cur.len) { err = EDE_GUARD; break; }
							if (MODE == EX_LEN) continue;
							if (a_o + alen > L) { err = EDE_OUT_RANGE; break; }
							for (uint32_t i = lane; i < alen; i += 64)
							{
								const uint32_t rb = ref_base(R, F.cur, a_c + i);
								if (rb > 3) lane_err = EDE_GUARD; else put(a_o + i, rb);
							}
						}
						F.cursor += atot; ocur += otot;
					}
					if (err) break;
					if (x.sl >= 64) break;
					if (__shfl(t, x.sl, 64) == T_MAIN_REF) F.to_main();
					else if ((err = F.to_alt(R, W, x.sl, lane))) break;
					todo = es_behind(todo, x.sl);
				}
				tup += (uint32_t)__popcll(W.starts); pos += W.p;
				if (!err && ocur > 0xffffffffull) err = EDE_TOO_LONG;
				if (!err) err = es_lane_err(lane_err);
			}
		}
	}
	if (!err) err = es_lane_err(lane_err);
#pragma unroll
	for (int d = 32; d > 0; d >>= 1) { const uint32_t o = __shfl_xor(diff, d, 64); diff = o < diff ? o : diff; }
	const bool ntup_bad = es_ntup && tup != es_ntup[r];
	bool mismatch = false;
	if (MODE == EX_CMP)
	{	// longer than the input, shorter, other tuple count, or a base differs: a bad read, not a malformed stream
		if (err == EDE_OUT_RANGE) { err = EDE_NONE; mismatch = true; }
		else if (!err) mismatch = ocur != L || ntup_bad || diff != 0xffffffffu;
	}
	else if (!err && ntup_bad) err = EDE_NTUP;
	if (lane != 0) return;
	if (MODE == EX_LEN) out_len[r] = err ? 0u : (uint32_t)ocur;
	if (err) { atomicAdd(&res->n_err, 1u); atomicMin(&res->first_err, ((unsigned long long)r << 32) | err); }
	else if (mismatch) { atomicAdd(&res->n_bad, 1u); atomicMin(&res->first_bad, ((unsigned long long)r << 32) | diff); }
}

Arena arena_of(const cl_reads* r) { return Arena{ r->packed.p, r->inv.p, r->word_off.p, r->lens.p, r->n_reads }; }
cl_status fetch_result(cl_ctx* ctx, const ExResult* d_res, ExResult& h, const char* who)
{
	HIP_TRY(ctx, hipGetLastError());
	HIP_TRY(ctx, hipMemcpyAsync(&h, d_res, sizeof(h), hipMemcpyDeviceToHost, ctx->stream));
	HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
	if (!h.n_err) return CL_OK;
	const uint32_t code = (uint32_t)h.first_err;
	return cl_fail(ctx, CL_E_INVALID, std::string(who) + ": " + std::to_string(h.n_err) + " malformed tuple stream(s), first: read " + std::to_string(h.first_err >> 32) + ": " +
		es_error_text(code));
}
} // namespace

extern "C" cl_status cl_es_expand(cl_ctx* ctx, const cl_reads* refs, const uint8_t* d_es, const uint64_t* d_es_off, const uint32_t* d_es_ntuples, uint32_t n_reads,
                                  uint8_t* d_codes, uint64_t cap, uint64_t* d_base_off, uint64_t* n_out)
{
	if (!ctx || !refs || !d_es_off || !d_base_off || !n_out || (n_reads && !d_es)) return cl_fail(ctx, CL_E_INVALID, "cl_es_expand: null argument");
	if (n_reads > 0x7fffffffu) return cl_fail(ctx, CL_E_UNSUPPORTED, "cl_es_expand: more than 2^31 - 1 reads in one call");      // (a block per read)
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	*n_out = 0;
	if (!n_reads) { HIP_TRY(ctx, hipMemsetAsync(d_base_off, 0, 8, ctx->stream)); HIP_TRY(ctx, hipStreamSynchronize(ctx->stream)); return CL_OK; }
	DevBuf<uint32_t> lens; DEV_ALLOC(ctx, lens, n_reads);
	DevBuf<ExResult> res; DEV_ALLOC(ctx, res, 1);
	const Arena R = arena_of(refs), none{ nullptr, nullptr, nullptr, nullptr, 0 };
	ExResult h;
	LAUNCH(ctx, k_es_result_init, 1, 1, res.p);
	LAUNCH_NAMED(ctx, "k_es_expand<len>", k_es_expand<EX_LEN>, n_reads, 64, R, none, d_es, d_es_off, d_es_ntuples, n_reads, lens.p, (uint8_t*)nullptr, (const uint64_t*)nullptr, res.p);
	CL_TRY(fetch_result(ctx, res.p, h, "cl_es_expand"));
	uint64_t total = 0;
	CL_TRY(dev_exclusive_scan_u64(ctx, lens.p, d_base_off, n_reads, &total));
	*n_out = total;
	if (total > cap || (total && !d_codes)) return cl_fail(ctx, CL_E_CAPACITY, "cl_es_expand: need " + std::to_string(total) + " bytes");
	LAUNCH_NAMED(ctx, "k_es_expand<store>", k_es_expand<EX_STORE>, n_reads, 64, R, none, d_es, d_es_off, d_es_ntuples, n_reads, (uint32_t*)nullptr, d_codes, (const uint64_t*)d_base_off, res.p);
	CL_TRY(fetch_result(ctx, res.p, h, "cl_es_expand"));
	cl_timing_collect(ctx);
	return CL_OK;
}

// cl_es_verify with the first differing base of the first bad read (~0u: its length or tuple count differs) and, for the achieved
// bytes/s of timed runs, the tuple bytes (0: not known)
cl_status cl_es_verify_at(cl_ctx* ctx, const cl_reads* reads, const cl_reads* refs, const uint8_t* d_es, const uint64_t* d_es_off, const uint32_t* d_es_ntuples,
                          uint64_t es_bytes, uint64_t* n_bad, uint32_t* first_bad, uint32_t* first_diff)
{
	if (!ctx || !reads || !refs || !d_es_off || !n_bad || !first_bad || (reads->n_reads && !d_es)) return cl_fail(ctx, CL_E_INVALID, "cl_es_verify: null argument");
	HIP_TRY(ctx, hipSetDevice(ctx->device));
	*n_bad = 0; *first_bad = 0xffffffffu;
	if (first_diff) *first_diff = 0xffffffffu;
	const uint32_t n = reads->n_reads;
	if (!n) return CL_OK;
	if (n > 0x7fffffffu) return cl_fail(ctx, CL_E_UNSUPPORTED, "cl_es_verify: more than 2^31 - 1 reads in one call");                 // (a block per read)
	DevBuf<ExResult> res; DEV_ALLOC(ctx, res, 1);
	LAUNCH(ctx, k_es_result_init, 1, 1, res.p);
	// algorithmic bytes: the tuple bytes, the reference bases fetched at 2 bits each (at most one per base of the input), the input's words and N masks
	const double bytes = (double)es_bytes + (double)reads->total_bases / 4 + (double)reads->total_words * 12;
	LAUNCHB_NAMED(ctx, "k_es_expand<compare>", bytes, k_es_expand<EX_CMP>, n, 64, arena_of(refs), arena_of(reads), d_es, d_es_off, d_es_ntuples, n, (uint32_t*)nullptr, (uint8_t*)nullptr,
		(const uint64_t*)nullptr, res.p);
	ExResult h;
	CL_TRY(fetch_result(ctx, res.p, h, "cl_es_verify"));
	cl_timing_collect(ctx);
	*n_bad = h.n_bad;
	if (h.n_bad) { *first_bad = (uint32_t)(h.first_bad >> 32); if (first_diff) *first_diff = (uint32_t)h.first_bad; }
	return CL_OK;
}

extern "C" cl_status cl_es_verify(cl_ctx* ctx, const cl_reads* reads, const cl_reads* refs, const uint8_t* d_es, const uint64_t* d_es_off, const uint32_t* d_es_ntuples,
                                  uint64_t* n_bad, uint32_t* first_bad)
{
	return cl_es_verify_at(ctx, reads, refs, d_es, d_es_off, d_es_ntuples, 0, n_bad, first_bad, nullptr);
}
