// Kernels over the two-stage scans: the closest-hit scan alone, renderer::render_flat, renderer::render.
// SCAN = 2: sp_cyl_scan.h scan_cylw (cylinder filter in f32, bit words, stage 2 shared by the wave)
// SCAN = 3: sp_cylm_scan.h scan_cylm (stage 1 on the f16 matrix pipe, one ray per lane, stage 2 shared by the wave), 256-thread workgroups
// SCAN = 4: the same scan in 512-thread workgroups with 512-triangle tiles (larger scenes)
#pragma once

#include "sp_cyl_scan.h"
#include "sp_cylm_both.h"

namespace sp {

struct ScanSrc {
	const void* reserved;    // the retired slab records' slot, left null: the members behind it keep their kernel-argument offsets, so every kernel keeps its listing
	CylStream cyl;           // cylinder records (k_cyl_scatter)
	CylStream cylm;          // cylinder records + matrix fragments (k_cylm_scatter), in the tile size of the scan that reads them
};

// threads per workgroup of the kernels below: the matrix-pipe scan shares its (larger) tiles between 8 waves
template <int SCAN> constexpr uint32_t scan_block() { return SCAN == 4 ? cylm512::kMThreads : 256u; }

// tmax / shadow: the bounded and the any-hit (shadow ray) forms of the scans (sp_cylm_scan.h, scan_cylm)
template <int R, int SCAN, bool BOUNDED = false>
SP_DEV void two_stage_scan(const KArgs& a, const ScanSrc& src, float rv, const RaySlots<R>& s, float (&bd)[R], int (&bi)[R],
                           const float* tmax = nullptr, bool shadow = false) {
	if constexpr (SCAN == 4) { static_assert(R == 1, "scan_cylm: one ray per lane"); cylm512::scan_cylm<BOUNDED>(a, src.cylm, rv, s, bd, bi, tmax, shadow); }
	else if constexpr (SCAN == 3) { static_assert(R == 1, "scan_cylm: one ray per lane"); cylm256::scan_cylm<BOUNDED>(a, src.cylm, rv, s, bd, bi, tmax, shadow); }
	else { static_assert(SCAN == 2, "SCAN: 2, 3 or 4"); scan_cylw<R, BOUNDED>(a, src.cyl, rv, s, bd, bi, tmax, shadow); }
}

// ---- the closest-hit scan alone with a two-stage scan; R rays per lane
template <int R, int SCAN>
__global__ void __launch_bounds__(scan_block<SCAN>(), SP_PT_WAVES) k_hit_filter(const KArgs a, const ScanSrc src2, const unsigned int* __restrict__ bounds,
                                                    const int* __restrict__ src_idx, int* __restrict__ out_idx, float* __restrict__ out_d) {
	const float rv = __uint_as_float(bounds[0]);
	RaySlots<R> s;
	uint32_t k[R];
#pragma unroll
	for (int r = 0; r < R; ++r) {
		k[r] = blockIdx.x * (scan_block<SCAN>() * R) + r * scan_block<SCAN>() + threadIdx.x;
		const bool valid = k[r] < a.n_rays;
		const uint32_t kk = valid ? k[r] : a.n_rays - 1;
		load_ray(a, kk, s.o[r], s.dir[r]);
		s.src[r] = src_idx ? src_idx[kk] : -1; s.act[r] = valid;
	}
	float bd[R]; int bi[R];
	two_stage_scan<R, SCAN>(a, src2, rv, s, bd, bi);
	uint32_t nsc = 0;
#pragma unroll
	for (int r = 0; r < R; ++r) if (k[r] < a.n_rays) { out_idx[k[r]] = bi[r]; out_d[k[r]] = bd[r]; nsc++; }
	wave_add_scans(a.scans, nsc);
}

// ---- renderer::render_flat with a two-stage scan; R pixels per lane
template <int R, int SCAN>
__global__ void __launch_bounds__(scan_block<SCAN>(), SP_PT_WAVES) k_flat_filter(const KArgs a, const ScanSrc src2, const unsigned int* __restrict__ bounds) {
	const float rv = __uint_as_float(bounds[0]);
	const uint32_t tid = threadIdx.x;
	RaySlots<R> s;
	uint32_t k[R];
	bool valid[R];
#pragma unroll
	for (int r = 0; r < R; ++r) {
		k[r] = blockIdx.x * (scan_block<SCAN>() * R) + r * scan_block<SCAN>() + tid;
		valid[r] = k[r] < a.n_rays;
		const uint32_t kk = valid[r] ? k[r] : a.n_rays - 1;
		load_ray(a, kk, s.o[r], s.dir[r]);
		s.src[r] = -1; s.act[r] = valid[r];
	}
	float bd[R]; int bi[R];
	two_stage_scan<R, SCAN>(a, src2, rv, s, bd, bi);
	uint32_t nsc = 0;
#pragma unroll
	for (int r = 0; r < R; ++r) {
		const uint32_t px = flat_px(a, bi[r]);
		if (valid[r]) { a.out_rgba[k[r]] = px; nsc++; }
	}
	wave_add_scans(a.scans, nsc);
}

// ---- renderer::render with the filter scan; R paths per lane advance in lock-step.
// SPLIT = false: the R slots of a lane are R different pixels (ray k0 + r*256).
// SPLIT = true : the R slots are R CONSECUTIVE SAMPLES of the same pixel (sample smp*R + r); their results are
//                added to the accumulator in sample order, so the sum is the reference's (cpu_renderer.cpp:74-76).
//                A workgroup then covers 256 pixels instead of 256*R: small shards still fill the chip.
// Per-path history (hit index and cos(theta) per depth) and the per-pixel accumulator are parked in a
// global work buffer between scans instead of being held in VGPRs through the scan loop: 52 B per slot,
// touched once per bounce, against ~10^5 VALU instructions per bounce.
//   work layout: hist[depth][k] = {idx, cos bits} (8 B), then acc[c][k] (3 floats), k < n_work
// With a trailing AccumArgs (progressive accumulation, sp_integrator.h) the running sum enters the slot's accumulator at the start
// and leaves it at the end -- with SPLIT only slot 0 carries it; a sample-chunked launch leaves both to k_resolve.
// With a trailing AdaptArgs (adaptive sampling) the same holds for S1, S2, parked in AdaptArgs::wst[2][n_work] (16 B per slot,
// touched once per sample, never inside the scan), and ray k is local pixel list[k] for the RNG and the running sums.
// With a SpecArgs (specular reflection, sp_integrator.h) a hit that took the mirror lobe carries kSpecBit in its history index: the
// slot stays 8 B per depth, and the unwind (and the next hit's MIS weight) reads the lobe back from there.
// With a NormArgs (smooth shading, sp_integrator.h) the barycentric coordinates are recomputed for the winning triangle after the
// scan (shade_normal), never inside its tile loops; a path whose bounce leaves the surface's upper side stops being active.
// With a TexArgs (textures, sp_integrator.h) the hit's albedo is computed once per hit after the scan (tex_albedo) and parked in
// TexArgs::A[5][3][n_work] (12 B per depth and slot) for the unwind.
template <int R, bool SPLIT, int SCAN, typename... Acc>
__global__ void __launch_bounds__(scan_block<SCAN>(), SP_PT_WAVES) k_pt_filter(const KArgs a, const ScanSrc src2, const unsigned int* __restrict__ bounds,
                                                   int2* __restrict__ hist, float* __restrict__ acc, uint32_t n_work, const Acc... acc_args) {
	const float rv = __uint_as_float(bounds[0]);
	const uint32_t tid = threadIdx.x;
	constexpr uint32_t B = scan_block<SCAN>();                // threads per workgroup
	const uint32_t k0 = blockIdx.x * (B * R) + tid;          // work-buffer slot of path r: k0 + r*B
	const uint32_t kstep = SPLIT ? 0u : B;                   // ray index of slot r: kr0 + r*kstep
	const bool chunked = a.n_chunks > 1;                     // blockIdx = chunk * px_blocks + pixel block
	const uint32_t pblk = chunked ? blockIdx.x % a.px_blocks : blockIdx.x;
	const uint32_t chunk = chunked ? blockIdx.x / a.px_blocks : 0u;
	const uint32_t kr0 = SPLIT ? pblk * B + tid : pblk * (B * R) + tid;
	constexpr bool adapt = IsAdapt<Acc...>::value;
	constexpr bool nee = IsNee<Acc...>::value;               // next-event estimation: L_d parked in NeeArgs::L (sp_integrator.h)
	static_assert(!nee || SCAN >= 2, "NEE needs the bounded form of the scan");
	constexpr bool mis = IsMis<Acc...>::value;               // MIS: D_d parked in NeeArgs::L for d = 0..4 (sp_integrator.h MisArgs)
	constexpr bool cam = IsCam<Acc...>::value;               // per-sample camera rays (sp_integrator.h CamArgs): KArgs::rays is not read
	constexpr bool spc = IsSpec<Acc...>::value;              // specular reflection (sp_integrator.h SpecArgs)
	static_assert(!spc || mis || !nee, "specular reflection: plain or NEE|MIS (DESIGN.md section 5.7)");
	constexpr bool smo = IsNorm<Acc...>::value;              // smooth shading (sp_integrator.h NormArgs)
	static_assert(!smo || ((mis || !nee) && SCAN >= 3), "smooth shading: plain or NEE|MIS, the default scan (DESIGN.md section 5.8)");
	constexpr bool gls = IsGlass<Acc...>::value;             // transparency (sp_integrator.h GlassArgs, in SpecArgs' place)
	static_assert(!gls || SCAN >= 3, "transparency: the default scan (DESIGN.md section 5.10)");
	constexpr bool env = IsEnv<Acc...>::value;               // environment lighting (sp_integrator.h EnvArgs, in GlassArgs' place)
	static_assert(!env || mis || !nee, "environment lighting: plain or NEE|MIS (DESIGN.md section 5.11)");
	constexpr bool glo = IsGloss<Acc...>::value;             // glossy reflection (sp_integrator.h GlossArgs, in EnvArgs' place)
	constexpr bool tex = IsTex<Acc...>::value;               // textures (sp_integrator.h TexArgs, in GlossArgs' place): the hit's albedo parked in TexArgs::A
	constexpr bool nmp = IsNmap<Acc...>::value;              // normal mapping (sp_integrator.h NmapArgs, in TexArgs' place, always with NormArgs): ns from the map
	static_assert(!nmp || smo, "a normal-mapped pack carries NormArgs (DESIGN.md section 5.16)");
	constexpr int hmask = HistMask<Acc...>::value;
	uint32_t pixel[R];
#pragma unroll
	for (int r = 0; r < R; ++r) {
		const uint32_t k = kr0 + r * kstep;
		const uint32_t kk = k < a.n_rays ? k : a.n_rays - 1;
		const uint32_t pk = local_px(kk, acc_args...);
		pixel[r] = (uint32_t)shard_pixel(a, pk);
#pragma unroll
		for (int c = 0; c < 3; ++c) acc[(size_t)c * n_work + k0 + r * B] = 0.0f;
		if constexpr (adapt) { adapt_args(acc_args...).wst[k0 + r * B] = 0.0; adapt_args(acc_args...).wst[(size_t)n_work + k0 + r * B] = 0.0; }
		if constexpr (HasAccum<Acc...>::value) {
			const AccumArgs& q = accum_args(acc_args...);
			const size_t ks = adapt ? pk : k;                    // index of the running sum
			if (q.sample_base && !chunked && (!SPLIT || r == 0) && k < a.n_rays) {
#pragma unroll
				for (int c = 0; c < 3; ++c) acc[(size_t)c * n_work + k0 + r * B] = q.sum[ks * 3 + c];
				if constexpr (adapt) {
					const AdaptArgs& d = adapt_args(acc_args...);
					d.wst[k0 + r * B] = d.s12[ks * 2]; d.wst[(size_t)n_work + k0 + r * B] = d.s12[ks * 2 + 1];
				}
			}
		}
	}
	// primary-hit reuse: cpu_renderer.cpp:74-76 starts every sample from the same vp.rays[idx], so the first
	// scan of all samples of a pixel has one result; the host ran it once per pixel (k_hit_filter) before this launch
	const bool reuse = !cam && a.prim_idx != nullptr;           // the host rejects reuse with camera samples
	uint32_t my_scans = 0;
	float pd[R]; int pi[R];
#pragma unroll
	for (int r = 0; r < R; ++r) {
		const uint32_t k = kr0 + r * kstep;
		const uint32_t kk = k < a.n_rays ? k : a.n_rays - 1;
		pd[r] = reuse ? a.prim_d[kk] : 0.0f;
		pi[r] = reuse ? a.prim_idx[kk] : -1;
	}

	uint32_t s0 = 0;                                         // global index of the launch's first sample
	if constexpr (HasAccum<Acc...>::value) s0 = accum_args(acc_args...).sample_base;
	const uint32_t n_iter = SPLIT ? (a.n_samples + R - 1) / R : a.n_samples;
	uint32_t it0 = 0, it1 = n_iter;
	if (chunked) {
		const uint32_t per = (n_iter + a.n_chunks - 1) / a.n_chunks;
		it0 = chunk * per < n_iter ? chunk * per : n_iter;
		it1 = it0 + per < n_iter ? it0 + per : n_iter;
	}
	for (uint32_t it = it0; it < it1; ++it) {
		RaySlots<R> s;
		int nh[R];                       // surface hits of this path so far
		uint32_t smp[R];
		bool live[R];                    // this slot carries a sample in this iteration
		bool ms[R];                      // environment: this path left the scene, its miss term is parked in EnvArgs::M
#pragma unroll
		for (int r = 0; r < R; ++r) {
			const uint32_t k = kr0 + r * kstep;
			smp[r] = SPLIT ? it * R + r : it;
			live[r] = (k < a.n_rays) && (smp[r] < a.n_samples);
			if constexpr (cam) camera_ray(cam_args(acc_args...), a.seed, pixel[r], s0 + smp[r], s.o[r], s.dir[r]);
			else load_ray(a, k < a.n_rays ? k : a.n_rays - 1, s.o[r], s.dir[r]);
			s.src[r] = -1; s.act[r] = live[r];
			nh[r] = 0;
			ms[r] = false;
		}
#pragma unroll 1
		for (int depth = 0; depth < (mis ? kMisDepths : nee ? kNeeDepths : 5); ++depth) {   // NEE: the 5th hit would carry nothing
			bool any_alive = false;
#pragma unroll
			for (int r = 0; r < R; ++r) any_alive |= s.act[r];
			if (!__syncthreads_or(any_alive ? 1 : 0)) break;
			float bd[R]; int bi[R];
			if (depth == 0 && reuse) {
#pragma unroll
				for (int r = 0; r < R; ++r) { bd[r] = pd[r]; bi[r] = pi[r]; }
			} else {
				two_stage_scan<R, SCAN, nee>(a, src2, rv, s, bd, bi);
#pragma unroll
				for (int r = 0; r < R; ++r) my_scans += s.act[r] ? 1u : 0u;
			}
			if constexpr (nee) {
				// one light sample per hit, then ONE block-uniform shadow scan for the slots that have a shadow ray (none: skipped)
				const NeeArgs& ne = nee_args(acc_args...);
				RaySlots<R> sh;
				float tmx[R];
				f3 nadj[R];
				bool hitr[R], any_sh = false;
				bool slr[R];                                     // specular: the hit takes the mirror lobe (no light sample)
				bool smr[R];                                     // smooth shading: nadj is an interpolated normal
#pragma unroll
				for (int r = 0; r < R; ++r) {
					hitr[r] = s.act[r] && (bi[r] >= 0);
					if constexpr (env) if (s.act[r] && bi[r] < 0) {         // the ray left the scene (depth > 0: the slot holds the hit of depth - 1)
						const bool full = depth == 0 || (hist[(size_t)(depth > 0 ? depth - 1 : 0) * n_work + k0 + r * B].x & kSpecBit) != 0;
						const f3 Em = env_miss<mis>(env_args(acc_args...).env, s.dir[r], full);
						float* Mp = env_args(acc_args...).M + k0 + r * B;
						Mp[0] = Em.x; Mp[n_work] = Em.y; Mp[(size_t)2 * n_work] = Em.z;
						ms[r] = true;
					}
					sh.o[r] = s.o[r]; sh.dir[r] = s.dir[r]; sh.src[r] = s.src[r]; sh.act[r] = false; tmx[r] = kMaxDist;
					nadj[r] = s.dir[r];
					slr[r] = false;
					smr[r] = false;
					if (hitr[r]) {
						const float* tn = a.tris + (size_t)bi[r] * 12 + 9;
						f3 n = mk3(tn[0], tn[1], tn[2]);
						if (dot3(n, s.dir[r]) > 0.0f) n = scale3(n, -1.0f);
						f3 ns = n;                                 // the shading normal
						if constexpr (smo) smr[r] = shade_normal(a.tris + (size_t)bi[r] * 12, norm_table(acc_args...) + (size_t)bi[r] * 9, s.o[r], s.dir[r], n, ns);
						if constexpr (nmp) nmap_hit(a, nmap_args(acc_args...), bi[r], s.o[r], s.dir[r], n, ns, smr[r]);
						nadj[r] = ns;
						[[maybe_unused]] f3 alb;                   // textures: the hit's albedo, parked for the unwind
						if constexpr (tex) {
							alb = tex_hit(a, tex_args(acc_args...), bi[r], s.o[r], s.dir[r]);
							float* Ap = tex_args(acc_args...).A + (size_t)depth * 3 * n_work + k0 + r * B;
							Ap[0] = alb.x; Ap[n_work] = alb.y; Ap[(size_t)2 * n_work] = alb.z;
						}
						const f3 x = add3(s.o[r], scale3(s.dir[r], bd[r]));
						f3 wd = s.dir[r], Lc = mk3(0.0f, 0.0f, 0.0f);
						float tm = kMaxDist;
						if constexpr (mis) {
							float* Lp = ne.L + (size_t)depth * 3 * n_work + k0 + r * B;
							// D_d = e_d w_b + L_d, assuming the shadow ray gets through; e_d w_b waits in depth 4's cells (written at
							// depth 4 only) in case it does not
							const float* m = a.mats + (size_t)bi[r] * 6;
							bool full = depth == 0;                    // e_d counts in full: the camera's hit, or the hit after a mirror bounce
							// the light sample is drawn in one of two places: before De with a table, after it without one.  Keep both: the
							// kernels without SpecArgs then hold the instructions they held before the element existed (tools/listing_diff.py)
							if constexpr (spc) {
								if (depth > 0) full = (hist[(size_t)(depth - 1) * n_work + k0 + r * B].x & kSpecBit) != 0;
								const float pm = spec_table(acc_args...)[bi[r]].w;
								slr[r] = spec_lobe(a.seed, pixel[r], s0 + smp[r], depth, pm);
								// an interface is a specular hit whatever its row of the specular table: no light sample; its own lobe is drawn
								// after the shadow scan
								if constexpr (gls) if (glass_table(acc_args...)[bi[r]].w > 0.0f) slr[r] = true;
								if constexpr (tex) sh.act[r] = depth < kNeeDepths && !slr[r] && nee_light<true, env, true>(a, ne, pixel[r], s0 + smp[r], depth, x, ns, bi[r], wd, tm, Lc, env_map(acc_args...), &alb);
								else sh.act[r] = depth < kNeeDepths && !slr[r] && nee_light<true, env>(a, ne, pixel[r], s0 + smp[r], depth, x, ns, bi[r], wd, tm, Lc, env_map(acc_args...));
								if constexpr (smo) sh.act[r] = sh.act[r] && smooth_light_ok(smr[r], wd, n);
								if (sh.act[r]) Lc = scale3(Lc, 1.0f / (1.0f - pm));   // L_d wD (a diffuse hit: p < 1)
							}
							const f3 De = full ? mk3(m[3], m[4], m[5]) : mis_emit(a, mis_tipdf(acc_args...), s.dir[r], bd[r], bi[r]);
							if constexpr (!spc) sh.act[r] = depth < kNeeDepths && nee_light<true>(a, ne, pixel[r], s0 + smp[r], depth, x, ns, bi[r], wd, tm, Lc);
							if constexpr (smo && !spc) sh.act[r] = sh.act[r] && smooth_light_ok(smr[r], wd, n);
							const f3 Dd = depth < kNeeDepths ? add3(De, sh.act[r] ? Lc : mk3(0.0f, 0.0f, 0.0f)) : De;
							Lp[0] = Dd.x; Lp[n_work] = Dd.y; Lp[(size_t)2 * n_work] = Dd.z;
							if (sh.act[r]) {
								float* Lq = ne.L + (size_t)kNeeDepths * 3 * n_work + k0 + r * B;
								Lq[0] = De.x; Lq[n_work] = De.y; Lq[(size_t)2 * n_work] = De.z;
							}
							sh.o[r] = x; sh.dir[r] = wd; sh.src[r] = bi[r]; tmx[r] = tm;
						} else {
							sh.act[r] = nee_light(a, ne, pixel[r], s0 + smp[r], depth, x, n, bi[r], wd, tm, Lc);
							sh.o[r] = x; sh.dir[r] = wd; sh.src[r] = bi[r]; tmx[r] = tm;
							float* Lp = ne.L + (size_t)depth * 3 * n_work + k0 + r * B;
							Lp[0] = sh.act[r] ? Lc.x : 0.0f; Lp[n_work] = sh.act[r] ? Lc.y : 0.0f; Lp[(size_t)2 * n_work] = sh.act[r] ? Lc.z : 0.0f;
						}
					}
					any_sh |= sh.act[r];
				}
				if (__syncthreads_or(any_sh ? 1 : 0)) {
					float sbd[R]; int sbi[R];
					two_stage_scan<R, SCAN, true>(a, src2, rv, sh, sbd, sbi, tmx, true);
#pragma unroll
					for (int r = 0; r < R; ++r) {
						my_scans += sh.act[r] ? 1u : 0u;
						if (sh.act[r] && sbi[r] >= 0) {                 // occluded
							float* Lp = ne.L + (size_t)depth * 3 * n_work + k0 + r * B;
							if constexpr (mis) {                       // D_d = e_d w_b
								const float* Lq = ne.L + (size_t)kNeeDepths * 3 * n_work + k0 + r * B;
								Lp[0] = Lq[0]; Lp[n_work] = Lq[n_work]; Lp[(size_t)2 * n_work] = Lq[(size_t)2 * n_work];
							} else {
								Lp[0] = 0.0f; Lp[n_work] = 0.0f; Lp[(size_t)2 * n_work] = 0.0f;
							}
						}
					}
				}
				// the bounce, exactly as without NEE
#pragma unroll
				for (int r = 0; r < R; ++r) {
					bool ended = false;                          // smooth shading: the bounce left the surface's upper side
					if (hitr[r]) {
						f3 nd;
						float ct = 0.0f;
						f3 ng = nadj[r];                         // smooth shading: the stored normal again, read after the shadow scan
						if constexpr (smo) {
							const float* tn = a.tris + (size_t)sh.src[r] * 12 + 9;
							ng = mk3(tn[0], tn[1], tn[2]);
							if (dot3(ng, s.dir[r]) > 0.0f) ng = scale3(ng, -1.0f);
						}
						if (spc && slr[r]) {
							nd = spec_reflect(s.dir[r], nadj[r]);
							if constexpr (smo) ended = smr[r] && (!(dot3(s.dir[r], nadj[r]) < 0.0f) || dot3(nd, ng) < 0.0f);
							if constexpr (glo) {                     // not on an interface: its bounce follows below
								const float al = rough_table(acc_args...)[sh.src[r]];
								if (al > 0.0f && !(glass_table(acc_args...)[sh.src[r]].w > 0.0f)) gloss_hit(a, pixel[r], s0 + smp[r], depth, al, s.dir[r], nadj[r], ng, smr[r], nd, ct, ended);
							}
						} else {
							double r1, r2;
							philox_uniforms(a.seed, pixel[r], s0 + smp[r], (uint32_t)depth, &r1, &r2);
							nd = rand_unit_vec(nadj[r], r1, r2);
							ct = dot3(nd, nadj[r]);
							if constexpr (smo) ended = smr[r] && dot3(nd, ng) < 0.0f;
						}
						bool tr = false;                             // transparency: the bounce is a transmission
						if constexpr (gls) {                         // an interface took the mirror's branch above (ct = 0): its bounce replaces the mirror's
							const float gi = glass_table(acc_args...)[sh.src[r]].w;
							if (gi > 0.0f) tr = glass_bounce(a, pixel[r], s0 + smp[r], depth, sh.src[r], gi, s.dir[r], nadj[r], smr[r], nd, ended);
						}
						s.o[r] = sh.o[r];
						s.dir[r] = nd;
						s.src[r] = sh.src[r];
						if constexpr (gls) hist[(size_t)depth * n_work + k0 + r * B] = make_int2(sh.src[r] | (slr[r] ? kSpecBit : 0) | (tr ? kTransBit : 0), (int)__float_as_uint(ct));
						else hist[(size_t)depth * n_work + k0 + r * B] = make_int2(spc && slr[r] ? sh.src[r] | kSpecBit : sh.src[r], (int)__float_as_uint(ct));
						nh[r] = depth + 1;
					}
					s.act[r] = hitr[r] && !ended;
				}
				continue;
			}
#pragma unroll
			for (int r = 0; r < R; ++r) {
				const bool hit = s.act[r] && (bi[r] >= 0);
				if constexpr (env) if (s.act[r] && bi[r] < 0) {      // the ray left the scene
					const f3 Em = env_miss<false>(env_args(acc_args...).env, s.dir[r], true);
					float* Mp = env_args(acc_args...).M + k0 + r * B;
					Mp[0] = Em.x; Mp[n_work] = Em.y; Mp[(size_t)2 * n_work] = Em.z;
					ms[r] = true;
				}
				bool ended = false;                              // smooth shading: the bounce left the surface's upper side
				if (hit) {
					const float* tn = a.tris + (size_t)bi[r] * 12 + 9;
					f3 n = mk3(tn[0], tn[1], tn[2]);
					if (dot3(n, s.dir[r]) > 0.0f) n = scale3(n, -1.0f);
					f3 ns = n;                                   // the shading normal
					bool sm = false;
					if constexpr (smo) sm = shade_normal(a.tris + (size_t)bi[r] * 12, norm_table(acc_args...) + (size_t)bi[r] * 9, s.o[r], s.dir[r], n, ns);
					if constexpr (nmp) nmap_hit(a, nmap_args(acc_args...), bi[r], s.o[r], s.dir[r], n, ns, sm);
					if constexpr (tex) {                         // the hit's albedo, parked for the unwind
						const f3 alb = tex_hit(a, tex_args(acc_args...), bi[r], s.o[r], s.dir[r]);
						float* Ap = tex_args(acc_args...).A + (size_t)depth * 3 * n_work + k0 + r * B;
						Ap[0] = alb.x; Ap[n_work] = alb.y; Ap[(size_t)2 * n_work] = alb.z;
					}
					bool sl = false;
					float gi = 0.0f;                             // transparency: the triangle's ior; > 0: an interface, a specular hit
					if constexpr (gls) {
						gi = glass_table(acc_args...)[bi[r]].w;
						sl = gi > 0.0f || spec_lobe(a.seed, pixel[r], s0 + smp[r], depth, spec_table(acc_args...)[bi[r]].w);
					} else if constexpr (spc) sl = spec_lobe(a.seed, pixel[r], s0 + smp[r], depth, spec_table(acc_args...)[bi[r]].w);
					f3 nd;
					float ct = 0.0f;
					bool tr = false;                             // transparency: the bounce is a transmission
					if (gls && gi > 0.0f) tr = glass_bounce(a, pixel[r], s0 + smp[r], depth, bi[r], gi, s.dir[r], ns, sm, nd, ended);
					else if (spc && sl) {
						nd = spec_reflect(s.dir[r], ns);
						if constexpr (smo) ended = sm && (!(dot3(s.dir[r], ns) < 0.0f) || dot3(nd, n) < 0.0f);
						if constexpr (glo) { const float al = rough_table(acc_args...)[bi[r]]; if (al > 0.0f) gloss_hit(a, pixel[r], s0 + smp[r], depth, al, s.dir[r], ns, n, sm, nd, ct, ended); }
					} else {
						double r1, r2;
						philox_uniforms(a.seed, pixel[r], s0 + smp[r], (uint32_t)depth, &r1, &r2);
						nd = rand_unit_vec(ns, r1, r2);
						ct = dot3(nd, ns);
						if constexpr (smo) ended = sm && dot3(nd, n) < 0.0f;
					}
					s.o[r] = add3(s.o[r], scale3(s.dir[r], bd[r]));
					s.dir[r] = nd;
					s.src[r] = bi[r];
					hist[(size_t)depth * n_work + k0 + r * B] = make_int2((spc && sl ? bi[r] | kSpecBit : bi[r]) | (gls && tr ? kTransBit : 0), (int)__float_as_uint(ct));
					nh[r] = depth + 1;
				}
				s.act[r] = hit && !ended;
			}
		}
#pragma unroll
		for (int r = 0; r < R; ++r) {
			const uint32_t kw = k0 + r * B;
			f3 rec = mk3(0.0f, 0.0f, 0.0f);
			if constexpr (env) if (ms[r]) {
				const float* Mp = env_args(acc_args...).M + kw;
				rec = mk3(Mp[0], Mp[n_work], Mp[(size_t)2 * n_work]);
			}
			for (int d = nh[r] - 1; d >= 0; --d) {
				const int2 hc = hist[(size_t)d * n_work + kw];
				const int id = spc ? hc.x & hmask : hc.x;
				const float* m = a.mats + (size_t)id * 6;
				f3 brdf = scale3(mk3(m[0], m[1], m[2]), kInvPi);
				if constexpr (tex) {
					const float* Ap = tex_args(acc_args...).A + (size_t)d * 3 * n_work + kw;
					brdf = scale3(mk3(Ap[0], Ap[n_work], Ap[(size_t)2 * n_work]), kInvPi);
				}
				f3 e = mk3(m[3], m[4], m[5]);
				if constexpr (mis) {                         // D_d
					const float* Lp = nee_args(acc_args...).L + (size_t)d * 3 * n_work + kw;
					e = mk3(Lp[0], Lp[n_work], Lp[(size_t)2 * n_work]);
				} else if constexpr (nee) {                  // (e_0 or 0) + L_d
					const float* Lp = nee_args(acc_args...).L + (size_t)d * 3 * n_work + kw;
					if (d > 0) e = mk3(0.0f, 0.0f, 0.0f);
					e = add3(e, mk3(Lp[0], Lp[n_work], Lp[(size_t)2 * n_work]));
				}
				if constexpr (glo) rec = gloss_unwind(glass_table(acc_args...), spec_table(acc_args...), hc.x, e, brdf, rec, __uint_as_float((uint32_t)hc.y));
				else if constexpr (gls) rec = glass_unwind(glass_table(acc_args...), spec_table(acc_args...), hc.x, e, brdf, rec, __uint_as_float((uint32_t)hc.y));
				else if constexpr (spc) rec = spec_unwind(spec_table(acc_args...)[id], (hc.x & kSpecBit) != 0, e, brdf, rec, __uint_as_float((uint32_t)hc.y));
				else rec = add3(e, scale3(scale3(mul3(brdf, rec), __uint_as_float((uint32_t)hc.y)), kInvP));
			}
			// cpu_renderer.cpp:75 accum += sample, in sample order: with SPLIT the slots are consecutive samples of one
			// pixel and are added to slot 0's accumulator one after the other (this loop is unrolled in order)
			if (live[r] && chunked) {
				float* p = a.samp + (size_t)smp[r] * 3 * a.samp_stride + (kr0 + r * kstep);
				p[0] = rec.x; p[a.samp_stride] = rec.y; p[(size_t)2 * a.samp_stride] = rec.z;
			} else if (live[r]) {
				const uint32_t ka = SPLIT ? k0 : kw;
#pragma unroll
				for (int c = 0; c < 3; ++c) {
					float* p = acc + (size_t)c * n_work + ka;
					*p = *p + (c == 0 ? rec.x : c == 1 ? rec.y : rec.z);
				}
				if constexpr (adapt) {                           // S1, S2 beside the accumulator, in the same order
					double* w = adapt_args(acc_args...).wst + ka;
					const double y = lum_proxy(rec.x, rec.y, rec.z);
					w[0] = w[0] + y;
					w[n_work] = w[n_work] + y * y;
				}
			}
		}
	}
#pragma unroll
	for (int r = 0; r < (SPLIT ? 1 : R); ++r) {
		const uint32_t k = kr0 + r * kstep;
		const uint32_t kw = k0 + r * B;
		if (k < a.n_rays && !chunked) {
			if constexpr (HasAccum<Acc...>::value) {
				const AccumArgs& q = accum_args(acc_args...);
				const size_t ks = adapt ? local_px(k, acc_args...) : k;
#pragma unroll
				for (int c = 0; c < 3; ++c) q.sum[ks * 3 + c] = acc[(size_t)c * n_work + kw];
				if constexpr (adapt) {
					const AdaptArgs& d = adapt_args(acc_args...);
					d.s12[ks * 2] = d.wst[kw]; d.s12[ks * 2 + 1] = d.wst[(size_t)n_work + kw];
					continue;                                    // the frame is resolved from sums and counts (k_adapt_resolve)
				}
			}
			const f3 av = scale3(mk3(acc[kw], acc[(size_t)n_work + kw], acc[(size_t)2 * n_work + kw]), a.inv_n);
			a.out_rgba[k] = clamped_rgba(av);
			if (a.out_accum) {
				a.out_accum[(size_t)k * 3 + 0] = av.x;
				a.out_accum[(size_t)k * 3 + 1] = av.y;
				a.out_accum[(size_t)k * 3 + 2] = av.z;
			}
		}
	}
	wave_add_scans(a.scans, my_scans);
}

} // namespace sp
