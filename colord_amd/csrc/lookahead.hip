// lookahead.hip — the pipeline of a pass of cl_compressor: chunks that the caller announces (cl_compressor_prepare) are taken through
// stage A by the encode lanes and through the coders' model-independent halves by the preparation workers while the caller's thread
// codes the chunks before them; cl_compressor_encode (stream.hip) takes a finished job from here and has the coders' hooks installed
// that carry the chunks ahead through their model halves.  One mutex (lane_mu) and one condition variable serve all hand-overs.
#include "compressor.hpp"

void LookAhead::stop()
{
	{ std::lock_guard<std::mutex> l(lane_mu); lane_stop = true; }
	lane_cv.notify_all();
	for (auto& t : lane_threads) if (t.joinable()) t.join();
	for (auto& t : prep_threads) if (t.joinable()) t.join();
	if (qprep_thread.joinable()) qprep_thread.join();
	lane_threads.clear();
	prepared.clear();                                // (buffers go back to the lanes' pools)
}
void LookAhead::report(size_t n_chunks) const
{
	fprintf(stderr, "[stream] %zu chunks: dna prepared ahead %u, evolved ahead %u; qual prepared ahead %u, evolved ahead %u; %zu lanes\n", n_chunks, n_dna_prep, n_dna_ahead, n_qual_prep, n_qual_ahead, lane_ctx.size());
	fprintf(stderr, "[stream] lanes: %.2f s in stage A, %.2f s waiting for the window; dna preparation: %.2f s working, %.2f s waiting; encode calls waited %.2f s for a lane, %.2f s for the dna preparation, %.2f s for the quality preparation\n",
		w_lane_work, w_lane_idle, w_prep_work, w_prep_idle, w_enc_lane, w_enc_prep, w_enc_qprep);
}

// ---- the workers ----------------------------------------------------------------------------------------------------
// Each one waits under lane_mu (`l`) until `ready` holds or the compressor stops (false: the worker ends; the wait is added to *idle) ...
template<class Ready> static bool wait_ready(LookAhead& la, std::unique_lock<std::mutex>& l, double* idle, Ready ready)
{
	Lap lap;
	la.lane_cv.wait(l, [&]() { return la.lane_stop || ready(); });
	if (idle) lap(*idle);
	return !la.lane_stop;
}
// ... works on its own context, timed as the caller's is ...
template<class Work> static cl_status work_on(cl_compressor* c, cl_ctx* ctx, Work work)
{
	ctx->timing = c->ctx->timing;
	ctx->verify = c->ctx->verify;
	ctx->edit_profile = c->ctx->edit_profile;
	ctx->overlaps = c->ctx->overlaps;
	ctx->mappings = c->ctx->mappings;
	ctx->cigars = c->ctx->cigars;
	ctx->cigars_coded = c->ctx->cigars_coded;
	ctx->pileup = c->ctx->pileup;
	const cl_status s = work();
	cl_timing_collect(ctx);
	return s;
}
// ... and hands over what it made: `set` under lane_mu, the kernel times of its context into `times`
template<class Set> static void publish(LookAhead& la, cl_ctx* ctx, std::map<std::string, KernelTime>& times, Set set)
{
	{ std::lock_guard<std::mutex> l(la.lane_mu); set(); times.swap(ctx->times); ctx->times.clear(); }
	la.lane_cv.notify_all();
}

static void lane_main(cl_compressor* c, cl_ctx* lane)
{
	LookAhead& la = c->la;
	for (;;)
	{
		size_t idx; Prepared* job;
		{
			std::unique_lock<std::mutex> l(la.lane_mu);
			// the lanes run at most (lanes + 2) chunks ahead of the coders: what they finish (tuple streams, ~1.5 GB per Gbase) waits in
			// HBM until it is coded; the slack evens out chunks whose stage A or coders happen to be slow
			if (!wait_ready(la, l, &la.w_lane_idle, [&]() { return !la.lane_queue.empty() && la.lane_queue.front() <= c->enc_chunk + la.lane_ctx.size() + 1; })) return;
			idx = la.lane_queue.front(); la.lane_queue.pop_front();
			job = la.prepared[idx].get();
		}
		Lap lap;
		const cl_status s = work_on(c, lane, [&]() { return compressor_tuple_streams(c, lane, idx, job->reads, job->packs.data(), (uint32_t)job->packs.size() - 1, *job); });
		publish(la, lane, job->times, [&]() { lap(la.w_lane_work); job->status = s; if (s != CL_OK) job->err = lane->err; job->done = true; });
	}
}

// The DNA coder's chain per chunk was: tuple walks -> triple slots -> stable sort by (family, context) -> context runs -> model
// evolution -> interval coding, all on the caller's stream — after the aligner work of round 3 THE critical chain of a pass
// (22.5 of 25.7 s busy).  Everything before the model evolution depends on the tuple streams only (and on two scalars that chain
// from walk to walk), so this worker does it for the chunks ahead, in order, on a context of its own; the caller's stream keeps
// evolution and coding.
static void prep_main(cl_compressor* c, cl_ctx* ctx)
{
	LookAhead& la = c->la;
	for (;;)
	{
		size_t idx; Prepared* job; uint32_t n = 0, types_in = 0, read_id_in = 0, types_out = 0; cl_status s = CL_OK;
		{	// one claim at a time: the scalars of chunk idx + 1 follow from those of chunk idx
			std::lock_guard<std::mutex> claim(la.prep_claim_mu);
			{
				std::unique_lock<std::mutex> l(la.lane_mu);
				const bool go = wait_ready(la, l, &la.w_prep_idle, [&]() {
					if (la.prep_broken || la.prep_next < c->enc_chunk) return true;      // (a chunk was coded without these workers: the chain of walk scalars is lost)
					auto it = la.prepared.find(la.prep_next);
					return it != la.prepared.end() && it->second->done && la.prep_next <= c->enc_chunk + la.prep_ctxs.size() + la.evolve_depth;     // (far enough ahead for the chunks that may be evolved ahead)
				});
				if (!go || la.prep_broken) return;
				if (la.prep_next < c->enc_chunk) { la.prep_broken = true; la.lane_cv.notify_all(); return; }
				idx = la.prep_next; job = la.prepared[idx].get();
				n = job->reads->n_reads; types_in = la.prep_types; read_id_in = la.prep_read_id;
			}
			types_out = types_in;
			if (job->status == CL_OK && n) s = cl_dna_batch_types(ctx, job->es.p, job->es_off.p, n, job->es_bytes, types_in, &types_out);
			{
				std::lock_guard<std::mutex> l(la.lane_mu);
				if (s == CL_OK && job->status == CL_OK) { la.prep_types = types_out; la.prep_read_id += n; }
				la.prep_next = idx + 1;
			}
			la.lane_cv.notify_all();
		}
		DnaWalked* W = nullptr; uint32_t walked_types = types_out;
		if (s == CL_OK && job->status == CL_OK && n)
		{
			s = work_on(c, ctx, [&]() { return cl_dna_prepare_batch(ctx, c->dna, c->refs, job->es.p, job->es_off.p, job->es_nt.p, n, types_in, read_id_in,
			                                                         job->parts.empty() ? nullptr : job->parts.data(), job->parts.empty() ? 0u : (uint32_t)job->parts.size() - 1, &W, &walked_types); });
			if (s == CL_OK && walked_types != types_out) s = cl_fail(ctx, CL_E_INVALID, "dna preparation: the read types of a chunk changed between the claim and the walk");
		}
		publish(la, ctx, job->dna_times, [&]() {
			if (s == CL_OK && job->status == CL_OK) job->walked = W;
			else { if (W) cl_dna_walked_free(W); if (job->status == CL_OK) la.prep_broken = true; }   // (the caller's thread walks this chunk itself and reports what fails)
			job->dna_done = true;
		});
	}
}

// The quality coder's chain per chunk — symbols -> stable sort by context -> context runs -> model evolution -> interval coding —
// became the critical one once the DNA coder's first half had moved to prep_main.  Its first three steps depend on the input only:
// this worker makes them for the chunks ahead (one or two), on a context of its own.
static void qprep_main(cl_compressor* c, cl_ctx* ctx)
{
	LookAhead& la = c->la;
	for (;;)
	{
		size_t idx; Prepared* job;
		{
			std::unique_lock<std::mutex> l(la.lane_mu);
			if (!wait_ready(la, l, nullptr, [&]() { return la.qprep_next < c->enc_chunk || (la.prepared.count(la.qprep_next) && la.qprep_next <= c->enc_chunk + 1 + la.evolve_depth); })) return;
			if (la.qprep_next < c->enc_chunk) { la.qprep_next = c->enc_chunk; continue; }   // (chunks coded without an announcement: nothing chains here, catch up)
			idx = la.qprep_next; job = la.prepared[idx].get();
		}
		QualPrepared* P = nullptr;
		if (job->d_quals && job->d_base_off && !job->parts.empty() && job->reads->n_reads)
		{
			const cl_status s = work_on(c, ctx, [&]() { return cl_qual_prepare_batch(ctx, c->qual, job->reads, job->d_quals, job->d_base_off, nullptr, job->parts.data(), (uint32_t)job->parts.size() - 1, &P); });
			if (s != CL_OK) P = nullptr;                                             // (the caller's thread prepares this chunk itself and reports what fails)
		}
		publish(la, ctx, job->q_times, [&]() { job->qprep = P; job->q_done = true; la.qprep_next = idx + 1; });
	}
}

// ---- announcing a chunk ---------------------------------------------------------------------------------------------
// a context for a worker in `slot`, kept with the caller's context for the next compressor (its pool is warm)
static cl_status make_worker_ctx(cl_ctx* ctx, cl_ctx*& slot, int prio, int role, const char* what)
{
	if (slot) return CL_OK;
	const cl_status s = cl_ctx_create(ctx->device, &slot);
	if (s != CL_OK) return cl_fail(ctx, s, std::string("cl_compressor_prepare: no context for ") + what);
	cl_ctx_set_priority(slot, prio, role);
	return CL_OK;
}
// The first announcement (chunk `idx`) sets the look-ahead up, under lane_mu.  The COLORD_HIP_* switches of the look-ahead are read
// here, once per compressor (not per process: a caller may change them between compressors).
static cl_status lookahead_setup(cl_compressor* c, size_t idx, bool long_parts)
{
	cl_ctx* ctx = c->ctx; LookAhead& la = c->la;
	// two lanes.  (A third one was measured at 50 Gbases: once 19.3 against 20.5 s per pass, then — same code but for the coders'
	// own streams — 23.5 against 20.3 s on one box, twice: the machine is shared by ~20 streams and whatever the lanes gain the
	// preparation threads lose.  COLORD_HIP_ENCODE_LANES overrides.)
	uint32_t lanes = 2;
	// Long coder parts (the reference's packs of 4 Mi symbols: the byte-identical mode) make the interval coders the bound of a
	// chunk — a dependent chain of 1.3 s per part: then the model halves of the next two chunks are done ahead so that the coders of
	// three chunks run side by side, and two lanes feed them easily.  With short parts (the bench's 64 Ki) the coders are no bound.
	la.evolve_depth = long_parts ? 2 : 0;
	if (const char* e = getenv("COLORD_HIP_ENCODE_LANES")) lanes = (uint32_t)std::min(4, std::max(1, atoi(e)));
	if (const char* e = getenv("COLORD_HIP_EVOLVE_DEPTH")) la.evolve_depth = (uint32_t)std::min(3, std::max(0, atoi(e)));
	la.no_evolve_ahead = getenv("COLORD_HIP_NO_EVOLVE_AHEAD") != nullptr;
	const int prio = getenv("COLORD_HIP_NO_STREAM_PRIO") ? 0 : 1;
	while (ctx->lanes.size() < lanes)
	{
		cl_ctx* x = nullptr;
		CL_TRY(make_worker_ctx(ctx, x, +prio, CL_ROLE_LANE, "an encode lane"));         // the lanes bound a pass: their queues are served first
		ctx->lanes.push_back(x);
	}
	la.lane_ctx.assign(ctx->lanes.begin(), ctx->lanes.begin() + lanes);
	for (cl_ctx* lane : la.lane_ctx) la.lane_threads.emplace_back(lane_main, c, lane);
	// the DNA preparation: only from the first chunk on (its walk scalars chain from chunk to chunk)
	if (idx == 0 && c->enc_chunk == 0 && !getenv("COLORD_HIP_NO_DNA_PREP"))
	{
		// ONE worker.  (Two, claiming alternate chunks, were measured in round 5 when this chain was the busiest queue of a pass — 87 %: each
		// one's sort took twice as long beside the other's, 18.7 against 18.7 s per pass: the machine is the bound, not the chain.)
		CL_TRY(make_worker_ctx(ctx, ctx->prep, -prio, CL_ROLE_PREP, "the DNA preparation thread"));   // (works ahead: takes what the lanes and coders leave)
		la.prep_ctxs.assign(1, ctx->prep);
		la.prep_next = 0; la.prep_on = true;
		cl_dna_coder_state(c->dna, &la.prep_types, &la.prep_read_id);
		for (cl_ctx* pc : la.prep_ctxs) la.prep_threads.emplace_back(prep_main, c, pc);
	}
	// the quality preparation: level 1 only (above, the contexts take flags from the edit scripts), quality context of its own
	if (c->qual && c->P.level <= 1 && c->qctx && c->qctx != ctx && !getenv("COLORD_HIP_NO_QUAL_PREP"))
	{
		CL_TRY(make_worker_ctx(ctx, ctx->qprep, -prio, CL_ROLE_PREP, "the quality preparation thread"));
		la.qprep_next = idx; la.qprep_on = true;
		la.qprep_thread = std::thread(qprep_main, c, ctx->qprep);
	}
	return CL_OK;
}

extern "C" cl_status cl_compressor_prepare_parts(cl_compressor* c, const cl_reads* reads, const uint32_t* h_pack_bounds, uint32_t n_packs, const uint32_t* h_part_bounds, uint32_t n_parts,
                                                 const uint8_t* d_quals, const uint64_t* d_base_off)
{
	if (!c || !reads || !h_pack_bounds) return CL_E_INVALID;
	cl_ctx* ctx = c->ctx; LookAhead& la = c->la;
	if (c->phase != 2) return cl_fail(ctx, CL_E_INVALID, "cl_compressor_prepare: call after refs_finish");
	std::unique_lock<std::mutex> l(la.lane_mu);
	const size_t idx = std::max(la.n_announced, c->enc_chunk);
	if (idx < c->enc_chunk || idx >= c->chunk_reads.size() || c->chunk_reads[idx] != reads->n_reads)
		return cl_fail(ctx, CL_E_INVALID, "cl_compressor_prepare: chunks must be announced in the order and sizes of pass 1, before they are encoded");
	if (la.lane_ctx.empty()) CL_TRY(lookahead_setup(c, idx, h_part_bounds && n_parts && (reads->total_bases + reads->n_reads) / n_parts >= (1u << 19)));
	auto job = std::make_unique<Prepared>();
	job->reads = reads; job->packs.assign(h_pack_bounds, h_pack_bounds + n_packs + 1);
	if (h_part_bounds && n_parts) job->parts.assign(h_part_bounds, h_part_bounds + n_parts + 1);
	job->d_quals = d_quals; job->d_base_off = d_base_off;
	la.prepared[idx] = std::move(job);
	la.lane_queue.push_back(idx);
	la.n_announced = idx + 1;
	l.unlock();
	la.lane_cv.notify_all();
	return CL_OK;
}
extern "C" cl_status cl_compressor_prepare(cl_compressor* c, const cl_reads* reads, const uint32_t* h_pack_bounds, uint32_t n_packs)
{
	return cl_compressor_prepare_parts(c, reads, h_pack_bounds, n_packs, nullptr, 0, nullptr, nullptr);
}

// ---- coding a chunk: the announced job and the coders' hooks ---------------------------------------------------------
cl_status lookahead_take(cl_compressor* c, const cl_reads* reads, std::unique_ptr<Prepared>& job)
{
	LookAhead& la = c->la; const size_t idx = c->enc_chunk;
	std::unique_lock<std::mutex> l(la.lane_mu);
	auto it = la.prepared.find(idx);
	if (it == la.prepared.end()) return CL_OK;
	Prepared* p = it->second.get();
	if (p->reads != reads) return cl_fail(c->ctx, CL_E_INVALID, "cl_compressor_encode: not the chunk that was announced for this position");
	Lap lap;
	la.lane_cv.wait(l, [&]() { return p->done; });
	lap(la.w_enc_lane);
	if (la.prep_on && !la.prep_broken) la.lane_cv.wait(l, [&]() { return p->dna_done || la.prep_broken; });
	lap(la.w_enc_prep);
	if (la.qprep_on && la.qprep_next <= idx) la.lane_cv.wait(l, [&]() { return p->q_done; });
	lap(la.w_enc_qprep);
	job = std::move(it->second); la.prepared.erase(it);
	return CL_OK;
}

// what the device could still give this process: free memory + what the shared pool holds without using it
static uint64_t avail_bytes(cl_ctx* ctx)
{
	size_t fr = 0, tot = 0;
	if (hipMemGetInfo(&fr, &tot) != hipSuccess) { (void)hipGetLastError(); return 0; }
	return fr + (ctx->pool.reserved - std::min(ctx->pool.reserved, ctx->pool.live_bytes));
}
// While chunk `idx`'s interval coders run (a dependent chain per part that nothing else on this stream can use: ~0.1 s with parts
// of 64 Ki symbols, 1.3 s with the reference's 4 Mi), the chunks after it — `upto` on, at most evolve_depth ahead, while the device
// has `floor_bytes` to give — are taken through their model half: evolution of the models, triples, their own interval coders
// started.  take(chunk), under lane_mu, says whether the chunk's prepared half is there and takes it; evolve(chunk) is the coder's
// cl_*_evolve_ahead with it.  Polled from a coder's before_tail hook: never a wait here, the chunk being coded is due.
enum class Half { none, not_yet, taken };
template<class Take, class Evolve> static cl_status evolve_ahead(cl_compressor* c, size_t idx, size_t& upto, uint32_t& n_ahead, uint64_t floor_bytes, Take take, Evolve evolve)
{
	LookAhead& la = c->la;
	if (la.no_evolve_ahead) return CL_OK;
	for (;;)
	{
		const size_t k = std::max(upto, idx + 1);
		if (k > idx + la.evolve_depth) return CL_OK;
		if (avail_bytes(c->ctx) < floor_bytes) return CL_OK;
		Prepared* nx = nullptr;
		{
			std::lock_guard<std::mutex> l(la.lane_mu);
			auto it = la.prepared.find(k);
			const Half h = it == la.prepared.end() ? Half::none : take(*it->second);
			if (h == Half::not_yet) return la.lane_stop ? CL_OK : CL_HOOK_RETRY;
			if (h == Half::none) return CL_OK;
			nx = it->second.get();
		}
		CL_TRY(evolve(*nx));
		++n_ahead; upto = k + 1;
	}
}

void lookahead_quality(cl_compressor* c, Prepared* job, const ChunkCoder& coder)
{
	LookAhead& la = c->la; cl_ctx* qctx = coder.qctx; const size_t idx = c->enc_chunk;
	if (coder.overlap && job && job->qprep && job->d_quals == coder.io.d_quals) { cl_qual_set_ahead(c->qual, job->qprep); job->qprep = nullptr; ++la.n_qual_prep; }
	if (job && qctx) merge_times(qctx->times, job->q_times);
	if (!coder.overlap || !la.qprep_on) return;
	cl_qual_set_before_tail(c->qual, [c, idx, qctx]() -> cl_status {
		LookAhead& la = c->la; QualPrepared* P = nullptr;
		return evolve_ahead(c, idx, la.qual_evolved_upto, la.n_qual_ahead, 24ull << 30,
			[&](Prepared& p) {
				if (p.parts.empty() || !p.d_quals) return Half::none;
				if (!p.q_done) return Half::not_yet;
				if (!p.qprep) return Half::none;
				P = p.qprep; p.qprep = nullptr; return Half::taken;
			},
			[&](Prepared& nx) { return cl_qual_evolve_ahead(qctx, c->qual, nx.reads, nx.d_quals, nx.d_base_off, nx.parts.data(), (uint32_t)nx.parts.size() - 1, P); });
	});
}

cl_status lookahead_dna(cl_compressor* c, Prepared* job)
{
	LookAhead& la = c->la; const size_t idx = c->enc_chunk;
	if (job)
	{
		if (job->status != CL_OK) return cl_fail(c->ctx, job->status, "encode lane: " + job->err);
		merge_times(c->ctx->times, job->times); merge_times(c->ctx->times, job->dna_times);
		if (job->walked) { cl_dna_set_ahead(c->dna, job->walked); job->walked = nullptr; ++la.n_dna_prep; }
	}
	// with the DNA preparation at work the chunks ahead are evolved (a chunk ahead holds ~12 GB of triples and coder output: hence the
	// floor); without it only the next chunk's tuple walk is made ahead (cl_dna_walk_ahead)
	cl_dna_set_before_tail(c->dna, [c, idx]() -> cl_status {
		LookAhead& la = c->la; bool prep; Prepared* nx = nullptr;
		{
			std::lock_guard<std::mutex> l(la.lane_mu);
			prep = la.prep_on && !la.prep_broken;
			auto it = la.prepared.find(idx + 1);
			if (!prep && it != la.prepared.end() && it->second->done && it->second->status == CL_OK && it->second->reads->n_reads) nx = it->second.get();
		}
		if (prep)
		{
			DnaWalked* W = nullptr;
			return evolve_ahead(c, idx, la.dna_evolved_upto, la.n_dna_ahead, 28ull << 30,
				[&](Prepared& p) {
					if (p.parts.empty()) return Half::none;
					if (!p.dna_done) return la.prep_broken ? Half::none : Half::not_yet;
					if (!p.walked || p.status != CL_OK) return Half::none;
					W = p.walked; p.walked = nullptr; return Half::taken;
				},
				[&](Prepared& p) { return cl_dna_evolve_ahead(c->ctx, c->dna, c->refs, p.es.p, p.es_off.p, p.es_nt.p, p.reads->n_reads, p.parts.data(), (uint32_t)p.parts.size() - 1, W); });
		}
		return nx ? cl_dna_walk_ahead(c->ctx, c->dna, c->refs, nx->es.p, nx->es_off.p, nx->es_nt.p, nx->reads->n_reads) : CL_OK;
	});
	return CL_OK;
}
