// encode_diag.hpp — the diagnostics of the edit-script encoder's driver (COLORD_HIP_GAP_DEBUG, _GAP_SHAPES, _QUAD_PROFILE, _WAVE_PROFILE,
// _WAVE_HEARTBEAT).  Included by encode_es.hip only, after its kernels and LevelBufs; the steps of the driver call these behind their
// switch (EncKnobs).  Each one waits for what it prints — a diagnostic run is not a timed run.  tests/test_gpu_cli.py and
// tools/giant_check.py parse the [gaps] lines: their text is fixed.
#pragma once
#include <algorithm>
#include <chrono>
#include <string>
#include <thread>
#include <vector>

namespace diag {
// COLORD_HIP_GAP_DEBUG: shapes of the wave-class gaps of the level (the list is ascending in log2 of the work)
static cl_status wave_class_shapes(cl_ctx* ctx, hipStream_t st, uint32_t lv, const LevelBufs& L, const uint32_t* hb, const uint32_t* list, uint32_t n_list)
{
	HIP_TRY(ctx, hipStreamSynchronize(st));
	std::vector<uint32_t> h_ids(n_list);
	HIP_TRY(ctx, hipMemcpy(h_ids.data(), list, (uint64_t)n_list * 4, hipMemcpyDeviceToHost));
	std::vector<GapRec> all(L.n_gaps);
	HIP_TRY(ctx, hipMemcpy(all.data(), L.gaps.p, (uint64_t)L.n_gaps * sizeof(GapRec), hipMemcpyDeviceToHost));
	double work = 0, steps = 0; std::string txt; uint64_t hist[8] = { 0 }; double hwork[8] = { 0 };
	for (uint32_t i = 0; i < n_list; ++i)
	{
		const GapRec& t = all[h_ids[n_list - 1 - i]];
		const uint32_t rows = t.kind == GK_FLANK ? t.ne : t.use, cols = t.kind == GK_FLANK ? t.use : t.ne;
		const double w = (double)((rows + 63) / 64) * cols, st_ = (double)((rows + 4095) / 4096) * (cols + 63);
		work += w; steps += st_;
		const int b = rows <= 256 ? 0 : rows <= 1024 ? 1 : rows <= 4096 ? 2 : rows <= 16384 ? 3 : 4;
		hist[b]++; hwork[b] += st_;
		if (i < 8) txt += " " + std::string(t.kind == GK_FLANK ? "F" : "I") + std::to_string(rows) + "x" + std::to_string(cols);
	}
	fprintf(stderr, "[gaps] level %u: classes 1-4 %u, quad %u, wave %u; wave class: block-columns %.3g, sweep steps %.3g; by rows <=256 %llu (%.3g steps) <=1024 %llu (%.3g) <=4096 %llu (%.3g) <=16384 %llu (%.3g) more %llu (%.3g); largest:%s\n",
		lv, hb[5] - hb[1], hb[6] - hb[5], n_list, work, steps, (unsigned long long)hist[0], hwork[0], (unsigned long long)hist[1], hwork[1], (unsigned long long)hist[2], hwork[2],
		(unsigned long long)hist[3], hwork[3], (unsigned long long)hist[4], hwork[4], txt.c_str());
	return CL_OK;
}
// COLORD_HIP_GAP_DEBUG: what the tile jobs did with the level's giant gaps
static void giant_line(uint32_t lv, const uint32_t* hb, uint32_t n_team_redo)
{
	fprintf(stderr, "[gaps] level %u: %u giant gaps by tile jobs (largest script %u symbols), %u back to the wave kernel\n", lv, hb[8] - hb[7], hb[N_CLASSES + 2], n_team_redo);
}
// COLORD_HIP_GAP_DEBUG: the level's gaps per class and per hand-over
static void level_line(const cl_ctx* ctx, uint32_t lv, const uint32_t* hb, uint32_t n_quad_redo, uint32_t n_team_redo)
{
	fprintf(stderr, "[gaps] level %u: per class %u %u %u %u %u %u %u %u; quad -> wave %u, giant -> wave %u; wave-pool redo rounds of the call so far %llu\n", lv, hb[1] - hb[0], hb[2] - hb[1],
		hb[3] - hb[2], hb[4] - hb[3], hb[5] - hb[4], hb[6] - hb[5], hb[7] - hb[6], hb[8] - hb[7], n_quad_redo, n_team_redo, (unsigned long long)ctx->gap_paths[10]);
}
// COLORD_HIP_GAP_SHAPES: shapes and edit distances of the aligned gaps by class — what a band (edlib.cpp:192-212) would save, what fits LDS
static cl_status gap_shapes(cl_ctx* ctx, uint32_t lv, const LevelBufs& L, uint64_t es_total)
{
	HIP_TRY(ctx, hipDeviceSynchronize());
	std::vector<GapRec> all(L.n_gaps); std::vector<char> hes(es_total + 16);
	HIP_TRY(ctx, hipMemcpy(all.data(), L.gaps.p, (uint64_t)L.n_gaps * sizeof(GapRec), hipMemcpyDeviceToHost));
	HIP_TRY(ctx, hipMemcpy(hes.data(), L.es.p, es_total, hipMemcpyDeviceToHost));
	struct Acc { uint64_t n = 0; double cells = 0, band = 0, band_ideal = 0; std::vector<uint32_t> nm, dpm; uint64_t ratio[11] = { 0 }; } acc[N_CLASSES + 1];
	for (const GapRec& g : all)
	{
		if (g.kind == GK_TRIVIAL) continue;
		const uint32_t rows = g.kind == GK_FLANK ? g.ne : g.use, cols = g.kind == GK_FLANK ? g.use : g.ne;      // (gap_class, restated for the host)
		const uint32_t cls = (rows <= 256 && cols <= 256) ? (rows + 63) / 64 : (rows <= QUAD_ROWS && rows + cols <= QUAD_SEQ && (uint64_t)((rows + 63) / 64) * (cols + 16) <= QUAD_CELLS) ? 5u
			: (rows > GIANT_ROWS && rows <= GIANT_MAX_ROWS && (uint64_t)((rows + 63) / 64) * cols >= GIANT_WORK && rows / 8 < cols) ? 7u : 6u;
		if (!cls || !rows || !cols) continue;
		uint32_t d = 0; for (uint32_t x = 0; x < g.es_len; ++x) d += hes[g.es_off + x] != 'M';
		Acc& a = acc[cls]; ++a.n;
		const double nb = (rows + 63) / 64; a.cells += nb * cols;
		// edlib's k-doubling (edlib.cpp:192-212: k = 64, 128, ... until the score fits) with Ukkonen's band of 2 k + |rows - cols| + 1 rows
		const double diff = rows > cols ? rows - cols : cols - rows;
		auto bandw = [&](double k) { return std::min(nb, std::ceil((2 * k + diff + 1) / 64.0) + 1); };
		double k = 64, cost = 0; while (k < d) { cost += bandw(k) * cols * 0.5; k *= 2; }   // (a failed round stops about half way)
		a.band += cost + bandw(k) * cols; a.band_ideal += bandw(d) * cols;
		a.nm.push_back(rows + cols); a.dpm.push_back((uint32_t)(1000.0 * d / std::max(rows, cols)));
		a.ratio[std::min<uint32_t>(10, (uint32_t)(20.0 * d / std::max(rows, cols)))]++;
	}
	for (uint32_t cls = 1; cls <= N_CLASSES; ++cls)
	{
		Acc& a = acc[cls]; if (!a.n) continue;
		std::sort(a.nm.begin(), a.nm.end()); std::sort(a.dpm.begin(), a.dpm.end());
		auto pc = [&](std::vector<uint32_t>& v, double p) { return v[std::min<size_t>(v.size() - 1, (size_t)(p * v.size()))]; };
		auto le = [&](uint32_t x) { return (double)(std::upper_bound(a.nm.begin(), a.nm.end(), x) - a.nm.begin()) / a.n; };
		fprintf(stderr, "[shapes] level %u class %u: %llu gaps, block-columns %.4g, k-doubling band %.4g (%.2f), band of the true distance %.4g (%.2f); rows+cols p50 %u p90 %u p99 %u p99.9 %u max %u; <=1536 %.4f <=2048 %.4f <=2730 %.4f <=4096 %.4f; d/len permille p10 %u p50 %u p90 %u p99 %u; by d/len in steps of 5%%:",
			lv, cls, (unsigned long long)a.n, a.cells, a.band, a.band / a.cells, a.band_ideal, a.band_ideal / a.cells, pc(a.nm, 0.5), pc(a.nm, 0.9), pc(a.nm, 0.99), pc(a.nm, 0.999), a.nm.back(),
			le(1536), le(2048), le(2730), le(4096), pc(a.dpm, 0.1), pc(a.dpm, 0.5), pc(a.dpm, 0.9), pc(a.dpm, 0.99));
		for (int i = 0; i < 11; ++i) fprintf(stderr, " %llu", (unsigned long long)a.ratio[i]);
		fprintf(stderr, "\n");
	}
	return CL_OK;
}
// COLORD_HIP_QUAD_PROFILE: the phases of the row kernel (waits for the launch on its stream)
static cl_status quad_profile(cl_ctx* ctx, hipStream_t side2, const unsigned long long* qp, uint32_t lv, uint32_t n_list, uint32_t waves)
{
	unsigned long long hp[16];
	HIP_TRY(ctx, hipStreamSynchronize(side2));
	HIP_TRY(ctx, hipMemcpy(hp, qp, 128, hipMemcpyDeviceToHost));
	const double q = (double)std::max<unsigned long long>(hp[9], 1);
	fprintf(stderr, "[quad rows, level %u] %u gaps in %llu quads on %u waves; us per quad: stage %.1f sweep %.1f walk %.1f convert %.1f refactor %.1f fetch+write %.1f; sweep steps per quad %.0f; walk iterations per quad %.0f, of which waited for new windows %.1f\n",
		lv, n_list, hp[9], waves, hp[0] / q / 100.0, hp[1] / q / 100.0, hp[2] / q / 100.0, hp[3] / q / 100.0, hp[4] / q / 100.0, hp[5] / q / 100.0, hp[10] / q, hp[6] / q, hp[7] / q);
	return CL_OK;
}
// COLORD_HIP_WAVE_PROFILE: the phases of one launch of the wave kernel and its slowest gap (waits for the launch)
static cl_status wave_profile(cl_ctx* ctx, hipStream_t st, const unsigned long long* prof, uint32_t lv, uint32_t n_list, uint32_t lanes, std::chrono::steady_clock::time_point t_launch)
{
	unsigned long long hp[16];
	HIP_TRY(ctx, hipStreamSynchronize(st));
	HIP_TRY(ctx, hipMemcpy(hp, prof, 128, hipMemcpyDeviceToHost));
	fprintf(stderr, "[slowest gap, level %u] kind %llu read symbols %llu reference symbols %llu: stage %.2f sweep %.2f path %.2f convert %.2f refactor %.2f ms\n", lv, hp[15], hp[14] >> 32, hp[14] & 0xffffffffull,
		hp[9] / 1e5, hp[10] / 1e5, hp[11] / 1e5, hp[12] / 1e5, hp[13] / 1e5);
	fprintf(stderr, "[wave phases, level %u, %u gaps, Mcycles of 100 MHz] alloc %llu stage %llu sweep %llu path %llu convert %llu refactor %llu fetch %llu; slowest gap %.2f ms (rank %llu from the largest); launch of %u waves %.1f ms\n", lv, n_list,
		hp[0] / 1000000, hp[1] / 1000000, hp[2] / 1000000, hp[3] / 1000000, hp[4] / 1000000, hp[5] / 1000000, hp[7] / 1000000, (double)(hp[6] >> 24) / 1e5, hp[6] & 0xffffffull, lanes, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_launch).count());
	return CL_OK;
}
// COLORD_HIP_WAVE_HEARTBEAT: host-visible progress words for the wave kernel, dumped by a watchdog thread if the kernel is still running
// after a while.  A debugging aid: the thread is detached and the mapped page is never freed.
static cl_status wave_heartbeat(cl_ctx* ctx, uint32_t** hbt_dev)
{
	uint32_t* hbt_host = nullptr;
	HIP_TRY(ctx, hipHostMalloc((void**)&hbt_host, 4096 * 4, hipHostMallocMapped));
	memset(hbt_host, 0, 4096 * 4);
	HIP_TRY(ctx, hipHostGetDevicePointer((void**)hbt_dev, hbt_host, 0));
	std::thread([hbt_host]() { for (int t = 0; t < 3; ++t) { std::this_thread::sleep_for(std::chrono::seconds(8)); fprintf(stderr, "[heartbeat]");
		for (int i = 0; i < 24; ++i) fprintf(stderr, " %u", hbt_host[i]); fprintf(stderr, "\n"); fflush(stderr); } }).detach();
	return CL_OK;
}
} // namespace diag
