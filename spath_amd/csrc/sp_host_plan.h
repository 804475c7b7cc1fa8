// The host-side arithmetic of libspath_hip.so that needs no device: the plan of a render launch (sample chunks, grids, work-buffer
// sizes) and the light tables of next-event estimation.  Plain integers and std::vector, no HIP: a host compiler builds this header
// alone, and tests/test_host_plan.py holds it to hand-derived plans and to the numpy light tables.  spath_hip.hip is its one user.
#pragma once
#include "spath_hip.h"

#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

namespace sp_host {
// R = paths per lane of a two-stage scan (0: not one), split = the R paths are consecutive samples of ONE pixel rather than R pixels,
// scan = the scan (2 = f32 cylinder filter, sp_cyl_scan.h; 3 = stage 1 on the f16 matrix pipe, sp_cylm_scan.h; 4 = its 512-thread shape)
struct TwoStage { int R; bool split; int scan; };
// what a checked render does (check_render): later steps read these, never `flags`.  Every bit but adapt and prog is set in path tracing only
struct Features { bool nee, mis, spec, glass, env, smooth, cam, adapt, prog, gloss, tex, nmap; };
constexpr uint64_t kChunkTargetBlocks = 262144;         // 256 x the 1024 resident workgroups (measured: profiles/r01_sample_chunks.log)
constexpr uint64_t kChunkMaxBytes = 16ull << 30;         // cap of the per-sample scratch buffer

// THE table of what the two-stage path-tracing kernels park per work slot (sp_scan_kernels.h), buffer by buffer.  work: the path
// history (5 x int2), the accumulator (3 floats), then NEE's L[4][3] or MIS's D[5][3]; adp_wst: adaptive sampling's S1, S2 (2 doubles);
// env_M: the miss term of an environment render (a glossy render's kernels carry a map, the context's black one if need be).  The chunk back-off's estimate and the allocations both read it: a feature that parks
// something per slot adds its line here, once
// tex_A: the albedo of hits 0..4 of a textured render, A[5][3] (a textured render's kernels carry a map as a glossy render's do)
constexpr size_t kSlotHist = 40, kSlotAcc = 12, kSlotNeeL = 48, kSlotMisD = 60, kSlotAdaptWst = 16, kSlotEnvM = 12, kSlotTexA = 60;
struct SlotBytes { size_t work, adp_wst, env_M, tex_A; };
constexpr SlotBytes slot_bytes(const Features& f) {
	return { kSlotHist + kSlotAcc + (f.mis ? kSlotMisD : f.nee ? kSlotNeeL : 0), f.adapt ? kSlotAdaptWst : 0, f.env || f.gloss || f.tex || f.nmap ? kSlotEnvM : 0,
	         f.tex || f.nmap ? kSlotTexA : 0 };     // a normal-mapped render's kernels are textured ones (NmapArgs is a TexArgs)
}

struct LaunchPlan {
	uint32_t chunks = 1;                         // sample chunks; > 1: the kernels write per-sample results to `samp`, k_resolve sums them
	uint32_t px_blocks = 0, samp_stride = 0;     // set with chunks > 1, like samp_bytes (0: no sample buffer)
	uint64_t samp_bytes = 0;
	uint32_t grid = 0, grid_px = 0, grid_pt = 0; // workgroups of the exact-only kernels and the BVH, of the one-scan kernels, of k_pt_filter
	uint32_t n_work = 0;                         // work slots: padded paths x chunks
	uint32_t n_launches = 1;                     // the path kernel and, with chunks, the resolve (the primary-hit pre-pass is the dispatch's)
	SlotBytes slot{};                            // bytes per work slot of each work-side buffer
	bool too_large = false;                      // n_work would not fit 32 bits: the caller refuses the launch
};

// Sample chunks: the filter kernels keep 1024 workgroups resident (256 CUs x 4); a launch of only a few times that many ends with a
// long tail (its time is that of the slowest workgroup, ~12 % above the mean when everything starts together), so small frames and
// multi-GPU shards are split along the samples as well.  forced: the SPHIP_FLAG_CHUNKS field (0 = choose); pt: path tracing; bthreads:
// threads per workgroup of the variant's kernels; samp_cap, work_cap: what the two buffers hold already; free_bytes(): the device's
// free memory or a negative value when it cannot tell, asked at most once and only when a buffer would have to grow (not on every
// frame of a running viewer).
template <typename FreeBytes>
LaunchPlan plan_launch(uint64_t n_rays, uint64_t n_samples, uint32_t forced, bool pt, const TwoStage& ts, uint32_t bthreads, const Features& f,
                       uint64_t samp_cap, uint64_t work_cap, FreeBytes&& free_bytes) {
	LaunchPlan p;
	p.slot = slot_bytes(f);
	const bool is_ts = ts.R != 0;
	const uint32_t slots = is_ts && ts.split ? (uint32_t)ts.R : 1u;                       // samples of one pixel per lane
	const uint32_t rays_per_block = is_ts && !ts.split ? bthreads * (uint32_t)ts.R : bthreads;
	const uint64_t chunk_target = kChunkTargetBlocks * 256u / bthreads;                   // the same number of resident-wave rounds
	const uint64_t lanes = (n_rays + 1023) / 1024 * 1024 * slots;                         // padded paths of one chunk
	if (pt && is_ts) {
		const uint64_t px_blocks = (n_rays + rays_per_block - 1) / rays_per_block;
		const uint64_t n_iter = (n_samples + slots - 1) / slots;
		if (forced) p.chunks = forced;
		else while (px_blocks * p.chunks < chunk_target && p.chunks < 128) p.chunks *= 2;
		if (p.chunks > n_iter) p.chunks = (uint32_t)n_iter;
		const uint64_t samp_bytes = n_samples * 12 * ((n_rays + 255) / 256 * 256);
		if (p.chunks > 1 && !forced) {
			// the split is an optimisation: it must never make a render fail that would fit unsplit (52 B per pixel).
			// Keep the scratch under the cap and under 90 % of what the device has free beyond the cached buffers.
			int64_t free_b = 0;
			bool asked = false;
			if (samp_bytes > kChunkMaxBytes) p.chunks = 1;
			while (p.chunks > 1) {
				const uint64_t work_bytes = lanes * p.chunks * (p.slot.work + p.slot.adp_wst + p.slot.env_M + p.slot.tex_A);
				const uint64_t need = (samp_bytes > samp_cap ? samp_bytes : 0) + (work_bytes > work_cap ? work_bytes : 0);
				if (need == 0) break;
				if (!asked) { asked = true; if ((free_b = free_bytes()) < 0) { p.chunks = 1; break; } }
				if (need <= (uint64_t)((double)free_b * 0.9)) break;
				p.chunks /= 2;
			}
		}
		if (p.chunks > 1) { p.px_blocks = (uint32_t)px_blocks; p.samp_stride = (uint32_t)((n_rays + 255) / 256 * 256); p.samp_bytes = samp_bytes; }
	}
	p.grid = (uint32_t)((n_rays + 255) / 256 * p.chunks);
	// one-scan modes (flat pass, hits) have no samples to share a lane: a split variant runs there with R pixels per lane
	const uint32_t rpb1 = is_ts ? bthreads * (uint32_t)ts.R : 256u;
	p.grid_px = (uint32_t)((n_rays + rpb1 - 1) / rpb1);
	p.grid_pt = (uint32_t)((n_rays + rays_per_block - 1) / rays_per_block * p.chunks);
	const uint64_t n_work = lanes * p.chunks;
	p.too_large = pt && is_ts && n_work > 0xffffffffull;
	p.n_work = (uint32_t)n_work;
	p.n_launches = p.chunks > 1 ? 2u : 1u;
	return p;
}

// ---- the light table of next-event estimation (include/spath_hip.h), built once per scene: emitters are the
// triangles with Esum = ((double)Er + Eg) + Eb > 0, weighted by w = A * Esum (A in double from the f32 vertices); the table lists those
// with w > 0 in ascending index with their running double sum cdf and ipdf = (float)(W / Esum), W = the total.  tipdf is MIS's pdf by
// triangle: the ipdf of the triangle's entry, 0 for a triangle not in the table.  The order of the double operations is the contract.
struct LightTable {
	std::vector<double> cdf, esum;
	std::vector<int> tri;
	std::vector<float> ipdf, tipdf;
	double W = 0.0;
	size_t bad_tri = SIZE_MAX;                   // != SIZE_MAX: emittance component bad_comp of this triangle is negative or not finite; no table
	int bad_comp = 0;
};

// ipdf of every triangle entry under the table's W (an entry beyond them, the map's, keeps 0), and tipdf from it
inline void set_light_pdfs(LightTable& t, size_t n_tris) {
	t.ipdf.assign(t.cdf.size(), 0.0f);
	t.tipdf.assign(n_tris, 0.0f);
	for (size_t k = 0; k < t.esum.size(); ++k) { t.ipdf[k] = (float)(t.W / t.esum[k]); t.tipdf[(size_t)t.tri[k]] = t.ipdf[k]; }
}

// tris: 12 floats per triangle (three vertices, the normal), mats: 6 (reflectance, emittance)
inline LightTable build_light_table(const float* tris, const float* mats, size_t n_tris) {
	LightTable t;
	for (size_t i = 0; i < n_tris; ++i) {
		const float* e = &mats[i * 6 + 3];
		for (int k = 0; k < 3; ++k)
			if (!(e[k] >= 0.0f) || !std::isfinite(e[k])) { t.bad_tri = i; t.bad_comp = k; return t; }
		const double es = ((double)e[0] + (double)e[1]) + (double)e[2];
		if (!(es > 0.0)) continue;
		const float* v = &tris[i * 12];
		const double e1[3] = { (double)v[3] - (double)v[0], (double)v[4] - (double)v[1], (double)v[5] - (double)v[2] };
		const double e2[3] = { (double)v[6] - (double)v[0], (double)v[7] - (double)v[1], (double)v[8] - (double)v[2] };
		const double cx = e1[1] * e2[2] - e1[2] * e2[1], cy = e1[2] * e2[0] - e1[0] * e2[2], cz = e1[0] * e2[1] - e1[1] * e2[0];
		const double w = (0.5 * std::sqrt((cx * cx + cy * cy) + cz * cz)) * es;
		if (!(w > 0.0) || !std::isfinite(w)) continue;
		t.W = t.W + w;
		t.cdf.push_back(t.W); t.tri.push_back((int)i); t.esum.push_back(es);
	}
	set_light_pdfs(t, n_tris);
	return t;
}

// the table of an environment render whose map has an entry: every triangle entry of `t` again with ipdf = (float)(W_env / Esum) under the
// total W_env that includes the map's weight, then the map's entry {cdf W_env, triangle -1, ipdf 0}
inline LightTable flagged_light_table(const LightTable& t, double W_env, size_t n_tris) {
	LightTable f = t;
	f.W = W_env;
	f.cdf.push_back(W_env); f.tri.push_back(-1);
	set_light_pdfs(f, n_tris);
	return f;
}

// The table on the device is one blob {double cdf[n]; int tri[n]; float ipdf[n]; float tipdf[n_tris]}: pack_light_table writes the
// layout and light_view reads it, and nothing else knows it
inline std::vector<char> pack_light_table(const LightTable& t) {
	const size_t n = t.cdf.size(), nt = t.tipdf.size();
	std::vector<char> blob(n * 16 + nt * 4);
	char* q = blob.data();
	auto put = [&q](const void* src, size_t bytes) { if (bytes) memcpy(q, src, bytes); q += bytes; };
	put(t.cdf.data(), n * 8); put(t.tri.data(), n * 4); put(t.ipdf.data(), n * 4); put(t.tipdf.data(), nt * 4);
	return blob;
}
struct LightView { const double* cdf; const int* tri; const float* ipdf; const float* tipdf; };
inline LightView light_view(const void* blob, size_t n) {
	const char* b = (const char*)blob;
	return { (const double*)b, (const int*)(b + n * 8), (const float*)(b + n * 12), (const float*)(b + n * 16) };
}

} // namespace sp_host
