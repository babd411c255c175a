// expand.hip — the inverse of a10-a12 on the device: a read rebuilt from its own tuple stream and the reference reads it points to.
// What CEncoder::Encode (encoder.cpp:1672-1691) wrote is read back as CDNACoder::Decode (dna_coder.cpp:234-437) applies it, without
// the entropy coder in between: cl_es_expand stores the bases, cl_es_verify compares them with the arena the streams were made from.
//
// A read's tuples refer to reference reads only, so reads expand independently: ONE WAVE PER READ, and within the read the wave
// takes the stream 64 bytes at a time (one byte per lane).  Per window:
//   1. tuple starts: a tuple is 1, 4 or 5 bytes long by its type nibble, and payload bytes look like anything, so the starts are
//      a chain — walked as a UNIFORM loop over three 64-bit ballots (one-byte types, four-byte, five-byte): a run of one-byte
//      tuples is one step (count-trailing-zeros), a multi-byte tuple one step: at most 2 x 16 steps per window, none per lane.  A
//      multi-byte tuple that crosses the window's end starts the next window.
//   2. every start lane has its tuple's output length and cursor advance (payloads by four lane shifts); alt-id / main-ref tuples
//      cut the window into stretches that share a reference (rare: a uniform loop over their ballot); within a stretch two wave
//      prefix sums place every tuple; unit tuples store / compare their one base; anchors are copied by the whole wave, a base per
//      lane straight from the packed words, in either orientation, whatever their alignment.
// So the time of a read grows with its stream bytes / 64 plus its anchor bases / 64, never with one lane's walk of the read.
// The table "alternative id -> orientation of its first appearance" (at most 64 entries) lives in one VGPR pair: lane i holds entry i.
//
// Bounds by construction (the kernel will meet the output of encoders that do not exist yet): a window never holds a byte at or past
// es_off[r + 1] and a tuple that would cross it is an error; every reference id is checked against the arena's read count before
// its length is loaded; every reference base comes through ref_base(), which answers 255 outside the read (an error, never an
// access); an anchor is checked against its reference's length and the read's measured length BEFORE its copy loop runs; every
// output index is checked against the measured length; a 65th alternative is an error.  A malformed stream gives its read an
// error code and the call CL_E_INVALID.
#include "common.hpp"
#include "objects.hpp"
#include "es_format.hpp"

namespace {
constexpr uint32_t EX_MAX_ALT = 64;
enum { EX_LEN = 0, EX_STORE = 1, EX_CMP = 2 };
enum { EXE_NONE = 0, EXE_EMPTY, EXE_START, EXE_TYPE, EXE_TRUNC, EXE_REF_ID, EXE_GUARD, EXE_VALUE, EXE_TOO_MANY_ALT, EXE_OUT_RANGE, EXE_TOO_LONG, EXE_NTUP, EXE_N };
const char* const EXE_TEXT[EXE_N] = { "", "empty stream", "first tuple is no start tuple", "tuple type not allowed inside an edit script", "tuple crosses the end of the stream",
	"reference id outside the reference arena", "position outside the reference read", "base value out of range", "more than 64 alternative references",
	"more bases than the length pass measured", "more than 2^32 - 1 bases", "tuple count differs from the one given" };

struct Arena { const uint64_t* packed; const uint32_t* inv; const uint64_t* word_off; const uint32_t* lens; uint32_t n; };
struct RefCursor { uint32_t id = 0, len = 0; uint64_t wo = 0; bool rev = false; };
// GetRefRead(id, rev)[pos] with the guard 255 (reference_reads.h:142-207); `c` was made from an id below the arena's read count
__device__ inline uint32_t ref_base(const Arena& R, const RefCursor& c, uint64_t pos)
{
	if (pos >= c.len) return 255;
	const uint32_t p = c.rev ? c.len - 1 - (uint32_t)pos : (uint32_t)pos;
	const uint32_t b = (uint32_t)(R.packed[c.wo + (p >> 5)] >> (62 - 2 * (p & 31))) & 3u;
	return c.rev ? 3u - b : b;
}
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
	uint32_t err = EXE_NONE;                                                    // uniform
	uint32_t lane_err = EXE_NONE, diff = 0xffffffffu;                           // per lane: what a base of mine ran into; first base of mine that differs
	uint64_t ocur = 0, tup = 0;                                                 // bases, tuples so far
	auto put = [&](uint64_t idx, uint32_t base) {
		if constexpr (MODE == EX_STORE) { if (idx < L) codes[o0 + idx] = (uint8_t)base; else lane_err = EXE_OUT_RANGE; }
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
	if (n == 0) err = EXE_EMPTY;
	else
	{
		EsReader rd{ s, s + n };
		uint32_t t0 = T_NONE, v1 = 0, v2 = 0;
		rd.next(t0, v1, v2);
		t0 = __builtin_amdgcn_readfirstlane(t0); v1 = __builtin_amdgcn_readfirstlane(v1); v2 = __builtin_amdgcn_readfirstlane(v2);
		if (t0 == T_START_PLAIN || t0 == T_START_PLAIN_N)
		{	// the rest of the stream is `plain` tuples: a lane per base
			if (n - 1 > 0xffffffffull) err = EXE_TOO_LONG;
			else
			{
				for (uint64_t i = lane; i < n - 1; i += 64)
				{
					const uint32_t b = s[1 + i];
					if ((b >> 4) != T_PLAIN) lane_err = EXE_TYPE; else if ((b & 0xf) > 4) lane_err = EXE_VALUE; else put(i, b & 0xf);
				}
				ocur = n - 1; tup = n;
			}
		}
		else if (t0 != T_START_ES) err = EXE_START;
		else if (n < 5) err = EXE_TRUNC;
		else if (v1 >= R.n) err = EXE_REF_ID;
		else
		{
			RefCursor mainc; mainc.id = v1; mainc.len = R.lens[v1]; mainc.wo = R.word_off[v1]; mainc.rev = v2 != 0;
			RefCursor cur = mainc;
			uint64_t cursor = 0, main_cursor = 0; bool is_main = true;
			uint32_t n_alt = 0, my_alt_id = 0, my_alt_rev = 0;                  // lane i: alternative i of this read and the orientation it came with first
			uint64_t pos = 5; tup = 1;
			while (!err && pos < n)
			{
				const uint32_t wn = n - pos < 64 ? (uint32_t)(n - pos) : 64u;   // bytes of this window: never one at or past the stream's end
				const uint32_t b = lane < wn ? (uint32_t)s[pos + lane] : 0xffu;
				const uint32_t t = b >> 4;
				const uint64_t m1 = __ballot(lane < wn && (t <= T_SUBST || t == T_MAIN_REF));
				const uint64_t m4 = __ballot(lane < wn && (t == T_ANCHOR || t == T_SKIP));
				const uint64_t m5 = __ballot(lane < wn && t == T_ALT_ID);
				uint64_t starts = 0; uint32_t p = 0;                            // p: bytes of the window that whole tuples take
				while (p < wn)
				{
					const uint64_t bit = 1ull << p;
					if (m1 & bit)
					{	// the run of one-byte tuples from here
						const uint64_t z = ~(m1 >> p);
						const uint32_t k = z ? (uint32_t)__builtin_ctzll(z) : 64u;
						starts |= (k >= 64 ? ~0ull : (1ull << k) - 1) << p; p += k;
					}
					else if (m4 & bit) { if (p + 4 > wn) break; starts |= bit; p += 4; }
					else if (m5 & bit) { if (p + 5 > wn) break; starts |= bit; p += 5; }
					else { err = EXE_TYPE; break; }
				}
				if (!err && p == 0) err = EXE_TRUNC;                            // (a window of 64 bytes holds any tuple: this one ends past the stream)
				if (err) break;
				const bool is_start = (starts >> lane) & 1;
				const uint32_t b1 = __shfl_down(b, 1, 64), b2 = __shfl_down(b, 2, 64), b3 = __shfl_down(b, 3, 64), b4 = __shfl_down(b, 4, 64);   // (a start's payload is inside the window)
				const uint32_t v28 = ((b & 0xf) << 24) | (b1 << 16) | (b2 << 8) | b3;
				const uint32_t id32 = (b1 << 24) | (b2 << 16) | (b3 << 8) | b4;
				const uint32_t outlen = !is_start ? 0u : (t == T_INS || t == T_MATCH || t == T_SUBST) ? 1u : t == T_ANCHOR ? v28 : 0u;
				const uint32_t adv = !is_start ? 0u : (t == T_DEL || t == T_MATCH || t == T_SUBST) ? 1u : (t == T_ANCHOR || t == T_SKIP) ? v28 : 0u;
				const uint64_t sw = starts & (m5 | __ballot(t == T_MAIN_REF));   // tuples that change the reference
				const uint64_t anch = starts & __ballot(t == T_ANCHOR);
				uint64_t todo = starts;
				while (todo && !err)
				{	// a stretch of tuples on one reference, then the tuple that ends it
					const uint64_t swm = todo & sw;
					const uint32_t sl = swm ? (uint32_t)__builtin_ctzll(swm) : 64u;
					const uint64_t seg = sl >= 64 ? todo : todo & ((1ull << sl) - 1);
					if (seg)
					{
						const bool in_seg = (seg >> lane) & 1;
						const uint32_t ol = in_seg ? outlen : 0u, ad = in_seg ? adv : 0u;     // (at most 16 multi-byte tuples of 28 bits: the sums fit 32 bits)
						const uint32_t oi = wave_incl_scan(ol), ai = wave_incl_scan(ad);
						const uint32_t otot = __shfl(oi, 63, 64), atot = __shfl(ai, 63, 64);
						if (MODE != EX_LEN && in_seg)
						{
							const uint64_t my_o = ocur + (oi - ol), my_c = cursor + (ai - ad);
							const uint32_t v = b & 0xf;
							if (t == T_INS) { if (v > 3) lane_err = EXE_VALUE; else put(my_o, v); }
							else if (t == T_MATCH) { const uint32_t rb = ref_base(R, cur, my_c); if (rb > 3) lane_err = EXE_GUARD; else put(my_o, rb); }
							else if (t == T_SUBST)
							{	// v-th of the three bases other than the reference's
								const uint32_t rb = ref_base(R, cur, my_c);
								if (rb > 3) lane_err = EXE_GUARD; else if (v > 2) lane_err = EXE_VALUE; else put(my_o, v + (v >= rb ? 1u : 0u));
							}
						}
						for (uint64_t am = seg & anch; am; am &= am - 1)
						{	// an anchor: the whole wave copies it
							const uint32_t l = (uint32_t)__builtin_ctzll(am);
							const uint32_t alen = __shfl(v28, l, 64);
							const uint64_t a_c = cursor + (__shfl(ai, l, 64) - alen), a_o = ocur + (__shfl(oi, l, 64) - alen);
							if (a_c + alen > cur.len) { err = EXE_GUARD; break; }
							if (MODE == EX_LEN) continue;
							if (a_o + alen > L) { err = EXE_OUT_RANGE; break; }
							for (uint32_t i = lane; i < alen; i += 64)
							{
								const uint32_t rb = ref_base(R, cur, a_c + i);
								if (rb > 3) lane_err = EXE_GUARD; else put(a_o + i, rb);
							}
						}
						cursor += atot; ocur += otot;
					}
					if (err) break;
					if (sl >= 64) break;
					if (__shfl(t, sl, 64) == T_MAIN_REF)
					{	// back to the main reference where it was left
						if (!is_main) { cur = mainc; cursor = main_cursor; is_main = true; }
					}
					else
					{
						const uint32_t id = __builtin_amdgcn_readfirstlane(__shfl(id32, sl, 64));
						const uint32_t orient = (__shfl(b, sl, 64) & 0xf) != 0 ? 1u : 0u;
						if (id >= R.n) { err = EXE_REF_ID; break; }
						if (is_main) { main_cursor = cursor; is_main = false; }
						const uint64_t hit = __ballot(lane < n_alt && my_alt_id == id);
						uint32_t rev;
						if (hit) rev = __shfl(my_alt_rev, (uint32_t)__builtin_ctzll(hit), 64);      // the orientation of its first appearance holds
						else
						{
							if (n_alt >= EX_MAX_ALT) { err = EXE_TOO_MANY_ALT; break; }
							if (lane == n_alt) { my_alt_id = id; my_alt_rev = orient; }
							++n_alt; rev = orient;
						}
						cur.id = id; cur.len = R.lens[id]; cur.wo = R.word_off[id]; cur.rev = rev != 0;
						cursor = 0;
					}
					todo &= ~(((1ull << sl) << 1) - 1);
				}
				tup += (uint32_t)__popcll(starts); pos += p;
				if (!err && ocur > 0xffffffffull) err = EXE_TOO_LONG;
				const uint64_t le = __ballot(lane_err != EXE_NONE);
				if (!err && le) err = __shfl(lane_err, (uint32_t)__builtin_ctzll(le), 64);
			}
		}
	}
	{
		const uint64_t le = __ballot(lane_err != EXE_NONE);
		if (!err && le) err = __shfl(lane_err, (uint32_t)__builtin_ctzll(le), 64);
	}
#pragma unroll
	for (int d = 32; d > 0; d >>= 1) { const uint32_t o = __shfl_xor(diff, d, 64); diff = o < diff ? o : diff; }
	const bool ntup_bad = es_ntup && tup != es_ntup[r];
	bool mismatch = false;
	if (MODE == EX_CMP)
	{	// longer than the input, shorter, other tuple count, or a base differs: a bad read, not a malformed stream
		if (err == EXE_OUT_RANGE) { err = EXE_NONE; mismatch = true; }
		else if (!err) mismatch = ocur != L || ntup_bad || diff != 0xffffffffu;
	}
	else if (!err && ntup_bad) err = EXE_NTUP;
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
		(code < EXE_N ? EXE_TEXT[code] : "?"));
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
