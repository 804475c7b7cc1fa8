// an acceleration structure behind the same C ABI -- OPT-IN (SPHIP_FLAG_ACCEL), never the
// default and never what bench.py's headline figure measures, because it changes the work definition: the reference
// has no acceleration structure (README.md:23) and tests every triangle.
//
// Structure: a linear BVH, built on the device (sp_bvh_build.h).  Triangles are sorted by the Morton code of their centroid, grouped four to a leaf, and
// the leaves (padded to a power of two) form a complete binary tree in heap order (root 1, children 2i and 2i+1), so
// parent / sibling / child links are index arithmetic and the tree is refitted bottom-up level by level.
// Traversal: one ray per lane, stackless with a bit trail (a set bit = "the far child of that level is still to do").
// Leaves run the SAME strict Moeller-Trumbore test as the brute-force scan (ray_tri_strict) on exact records
// that carry the triangle's ORIGINAL index, and hits are compared lexicographically by (d, original index), which
// is the reference's "first strictly smaller d wins, ascending index" rule (cpu_renderer.cpp:44) in any visiting order.
//
// Parity: the box test is conservative (boxes inflated, comparisons inclusive), so every GEOMETRIC hit the reference
// finds is found with the same index and the same distance bits.  What a bounding-volume cull cannot reproduce are
// the reference's noise accepts (a ray almost coplanar with a far-away triangle: a and s.h are both rounding noise and
// u, v land in [0,1] by chance -- DESIGN.md section 8).  tests/test_hip_accel.py measures how rare those are;
// tests/test_hip_bvh_walk.py holds every ray to the oracle and every difference to that explanation (float64 barycentrics outside).
#pragma once

#include "sp_kernels.h"

namespace sp {

struct BvhArgs {
	const float4* nodes;     // 2 x float4 per node, heap order, index 0 unused: {lo.xyz, hi.x} {hi.yz, -, -}
	const float4* leaf_rec;  // 3 x float4 per sorted triangle: v0, e1, e2 (exact records), 4 triangles per leaf
	const int*    leaf_idx;  // original triangle index per sorted triangle, -1 for padding
	uint32_t n_leaves;       // power of two
	uint32_t first_leaf;     // == n_leaves (heap index of leaf 0)
	const uint32_t* meta;    // device words of the builder (sp_bvh_build.h); meta[8] = n_big: triangles too large for the tree (room walls,
	                         // ground planes): sorted records [4*n_leaves, 4*n_leaves + n_big) are tested for every ray before the walk,
	                         // which also gives the walk a tight cull distance from the start
};

// inclusive slab test; NaNs from 0 * inf drop out because v_min/v_max return the non-NaN operand
SP_DEV bool box_hit(const float4 a, const float4 b, f3 o, f3 inv, float tbest, float& tnear) {
	const float x0 = (a.x - o.x) * inv.x, x1 = (a.w - o.x) * inv.x;
	const float y0 = (a.y - o.y) * inv.y, y1 = (b.x - o.y) * inv.y;
	const float z0 = (a.z - o.z) * inv.z, z1 = (b.y - o.z) * inv.z;
	const float tmin = fmaxf(fmaxf(fminf(x0, x1), fminf(y0, y1)), fmaxf(fminf(z0, z1), 0.0f));
	const float tmax = fminf(fminf(fmaxf(x0, x1), fmaxf(y0, y1)), fminf(fmaxf(z0, z1), tbest));
	tnear = tmin;
	// (a.x <= a.w) is false for the inverted boxes of empty padding subtrees, which the slab arithmetic alone would
	// read as infinitely large
	return (a.x <= a.w) && (tmin <= tmax * 1.00001f + 1e-30f);
}

// tmax < kMaxDist, any_hit: the shadow form -- only hits with d < tmax count, and the walk stops at the first one
// (SELFTEST only gives the test kernel at the end of this file an instantiation of its own: the one the render kernels share then keeps
// exactly its call sites, none of which asks for the counts, and their code does not move -- tools/listing_diff.py)
template <bool SELFTEST = false>
SP_DEV void scan_bvh(const BvhArgs& B, f3 o, f3 dir, int src, float& best_d, int& best_i, uint32_t* steps_out = nullptr, uint32_t* leaves_out = nullptr,
                     float tmax = kMaxDist, bool any_hit = false) {
	uint32_t n_steps = 0, n_leaves = 0;
	float bd = tmax;
	int bi = -1;
	const f3 inv = mk3(1.0f / dir.x, 1.0f / dir.y, 1.0f / dir.z);
	for (uint32_t j = 4u * B.n_leaves, e = 4u * B.n_leaves + B.meta[8]; j < e; ++j) {       // wave-uniform loop: scalar loads
		const int orig = B.leaf_idx[j];
		const float4 q0 = B.leaf_rec[3 * j], q1 = B.leaf_rec[3 * j + 1], q2 = B.leaf_rec[3 * j + 2];
		const float d = ray_tri_strict(o, dir, mk3(q0.x, q0.y, q0.z), mk3(q0.w, q1.x, q1.y), mk3(q1.z, q1.w, q2.x));
		const bool take = (orig != src) && (d > 0.0f) && ((d < bd) || (d == bd && orig < bi));
		bd = take ? d : bd;
		bi = take ? orig : bi;
	}
	if (any_hit && bi >= 0) { best_d = bd; best_i = bi; return; }
	uint32_t node = 1, trail = 0;
	// Every step either descends one level or retires one pending sibling, so the walk visits each node at most once;
	// the explicit bound is a belt-and-braces exit condition (a wave that never finishes can take the whole GPU down).
	// A little slack on the cull distance: a box may be entered a few ulps after the hit distance of a triangle inside it.
	for (uint32_t steps = 0, max_steps = 4u * B.n_leaves + 64u; steps < max_steps; ++steps) {
		bool descended = false;
		++n_steps;
		if (node < B.first_leaf) {
			const uint32_t c0 = 2 * node, c1 = c0 + 1;
			float t0, t1;
			const float cull = bd * 1.00001f;
			const bool h0 = box_hit(B.nodes[2 * c0], B.nodes[2 * c0 + 1], o, inv, cull, t0);
			const bool h1 = box_hit(B.nodes[2 * c1], B.nodes[2 * c1 + 1], o, inv, cull, t1);
			if (h0 | h1) {
				const bool both = h0 & h1;
				const bool first1 = both ? (t1 < t0) : h1;
				node = first1 ? c1 : c0;
				trail = (trail << 1) | (both ? 1u : 0u);
				descended = true;
			}
		} else {
			const uint32_t leaf = node - B.first_leaf;
			++n_leaves;
#pragma unroll
			for (int k = 0; k < 4; ++k) {
				const uint32_t j = leaf * 4 + k;
				const int orig = B.leaf_idx[j];
				const float4 q0 = B.leaf_rec[3 * j], q1 = B.leaf_rec[3 * j + 1], q2 = B.leaf_rec[3 * j + 2];
				const float d = ray_tri_strict(o, dir, mk3(q0.x, q0.y, q0.z), mk3(q0.w, q1.x, q1.y), mk3(q1.z, q1.w, q2.x));
				const bool take = (orig >= 0) && (orig != src) && (d > 0.0f) && ((d < bd) || (d == bd && orig < bi));
				bd = take ? d : bd;
				bi = take ? orig : bi;
			}
			if (any_hit && bi >= 0) break;
		}
		if (!descended) {
			// pop: climb to the deepest level whose far child is still pending and go to that sibling -- unless the best
			// distance found meanwhile already rules its box out (the box was tested when it was pushed, against an older best)
			bool found = false;
			while (trail != 0) {
				const int up = __builtin_ctz(trail);     // levels to climb
				node >>= up;
				trail >>= up;
				node ^= 1u;                               // the pending (far) sibling
				trail ^= 1u;                              // ... is now taken
				float tn;
				if (box_hit(B.nodes[2 * node], B.nodes[2 * node + 1], o, inv, bd * 1.00001f, tn)) { found = true; break; }
			}
			if (!found) break;
		}
	}
	best_d = bd;
	best_i = bi;
	if (steps_out) { *steps_out = n_steps; *leaves_out = n_leaves; }
}

// kernels: the same integrator / flat / hit bodies as the exact scans (sp_kernels.h), with the BVH as the scan; what the bodies
// share is in sp_integrator.h
// (a trailing AccumArgs: progressive accumulation in path-tracing mode; AdaptArgs: adaptive sampling; sp_integrator.h)
template <int MODE /* 0 flat, 1 pt, 2 hits */, typename... Acc>
__global__ void __launch_bounds__(256) k_accel(const KArgs a, const BvhArgs B, const int* __restrict__ src_idx,
                                               int* __restrict__ out_idx, float* __restrict__ out_d, const Acc... acc_args) {
	const uint32_t k = blockIdx.x * 256u + threadIdx.x;
	const bool valid = k < a.n_rays;
	const uint32_t kk = valid ? k : a.n_rays - 1;
	constexpr bool cam = IsCam<Acc...>::value;         // per-sample camera rays (sp_integrator.h CamArgs): KArgs::rays is not read
	f3 po = mk3(0.0f, 0.0f, 0.0f), pdir = po;
	if constexpr (!cam) {                              // load_ray, written out: the call moves this kernel's instructions (tools/listing_diff.py)
		const float* r = a.rays + (size_t)kk * 6;
		po = mk3(r[0], r[1], r[2]); pdir = mk3(r[3], r[4], r[5]);
	}
	if (MODE == 2) {
		float bd; int bi;
#ifdef SP_BVH_STATS
		uint32_t st = 0, lv = 0;
		scan_bvh(B, po, pdir, src_idx ? src_idx[kk] : -1, bd, bi, &st, &lv);
		wave_add_scans(a.scans + 1, st); wave_add_scans(a.scans + 2, lv);
#else
		scan_bvh(B, po, pdir, src_idx ? src_idx[kk] : -1, bd, bi);
#endif
		if (valid) { out_idx[k] = bi; out_d[k] = bd; }
		wave_add_scans(a.scans, valid ? 1u : 0u);
		return;
	}
	if (MODE == 0) {
		float bd; int bi;
		scan_bvh(B, po, pdir, -1, bd, bi);
		const uint32_t px = flat_px(a, bi);
		if (valid) a.out_rgba[k] = px;
		wave_add_scans(a.scans, valid ? 1u : 0u);
		return;
	}
	constexpr bool adapt = IsAdapt<Acc...>::value;     // adaptive: ray k is local pixel list[k] (sp_integrator.h AdaptArgs)
	constexpr bool nee = IsNee<Acc...>::value;         // next-event estimation (sp_integrator.h NeeArgs)
	constexpr bool mis = IsMis<Acc...>::value;         // MIS on top of it (sp_integrator.h MisArgs): the folded terms D_0..D_4
	constexpr bool spc = IsSpec<Acc...>::value;        // specular reflection (sp_integrator.h SpecArgs): kSpecBit in hidx marks a mirror bounce
	static_assert(!spc || mis || !nee, "specular reflection: plain or NEE|MIS (DESIGN.md section 5.7)");
	constexpr bool smo = IsNorm<Acc...>::value;        // smooth shading (sp_integrator.h NormArgs): ns of shade_normal shades, n guards
	static_assert(!smo || mis || !nee, "smooth shading: plain or NEE|MIS (DESIGN.md section 5.8)");
	constexpr bool gls = IsGlass<Acc...>::value;       // transparency (sp_integrator.h GlassArgs, in SpecArgs' place): kTransBit beside kSpecBit
	constexpr bool env = IsEnv<Acc...>::value;         // environment lighting (sp_integrator.h EnvArgs, in GlassArgs' place): a miss carries the map's radiance
	static_assert(!env || mis || !nee, "environment lighting: plain or NEE|MIS (DESIGN.md section 5.11)");
	constexpr bool glo = IsGloss<Acc...>::value;       // glossy reflection (sp_integrator.h GlossArgs, in EnvArgs' place): the weight g in the mirror hit's cosine slot
	constexpr bool tex = IsTex<Acc...>::value;         // textures (sp_integrator.h TexArgs, in GlossArgs' place): the hit's albedo per depth in hA
	constexpr bool nmp = IsNmap<Acc...>::value;        // normal mapping (sp_integrator.h NmapArgs, in TexArgs' place, always with NormArgs): ns from the map
	static_assert(!nmp || smo, "a normal-mapped pack carries NormArgs (DESIGN.md section 5.16)");
	constexpr int hmask = HistMask<Acc...>::value;
	const uint32_t pk = adapt ? local_px(kk, acc_args...) : kk;
	const uint32_t pixel = (uint32_t)shard_pixel(a, pk);
	uint32_t my_scans = 0;
	f3 accum = mk3(0.0f, 0.0f, 0.0f);
	double s1 = 0.0, s2 = 0.0;
	uint32_t s0 = 0;                                  // global index of the launch's first sample
	if constexpr (adapt) {
		const AdaptArgs& q = adapt_args(acc_args...);
		s0 = q.sample_base;
		if (s0 && valid) {
			accum = mk3(q.sum[(size_t)pk * 3 + 0], q.sum[(size_t)pk * 3 + 1], q.sum[(size_t)pk * 3 + 2]);
			s1 = q.s12[(size_t)pk * 2]; s2 = q.s12[(size_t)pk * 2 + 1];
		}
	} else if constexpr (HasAccum<Acc...>::value) {
		const AccumArgs& q = accum_args(acc_args...);
		s0 = q.sample_base;
		if (s0 && valid) accum = mk3(q.sum[(size_t)k * 3 + 0], q.sum[(size_t)k * 3 + 1], q.sum[(size_t)k * 3 + 2]);
	}
	for (uint32_t s = 0; s < a.n_samples; ++s) {
		f3 o = po, dir = pdir;
		if constexpr (cam) camera_ray(cam_args(acc_args...), a.seed, pixel, s0 + s, o, dir);
		int src = -1, hidx[5];
		float hcos[5];
		f3 hL[kNeeDepths];
		f3 hD[kMisDepths];
		f3 hA[5];                                       // textures: the albedo of hits 0..4
		int nh = 0;
		bool alive = valid;
		f3 Em = mk3(0.0f, 0.0f, 0.0f);                  // environment: what the ray that left the scene carries
#pragma unroll
		for (int depth = 0; depth < (mis ? kMisDepths : nee ? kNeeDepths : 5); ++depth) {
			if (alive) {
				float bd; int bi;
				scan_bvh(B, o, dir, src, bd, bi);
				my_scans++;
				if (bi >= 0) {
					const float* tn = a.tris + (size_t)bi * 12 + 9;
					f3 n = mk3(tn[0], tn[1], tn[2]);
					if (dot3(n, dir) > 0.0f) n = scale3(n, -1.0f);
					f3 ns = n;                                    // the shading normal
					bool sm = false, ended = false;               // smooth shading: a bounce below the surface ends the path
					if constexpr (smo) sm = shade_normal(a.tris + (size_t)bi * 12, norm_table(acc_args...) + (size_t)bi * 9, o, dir, n, ns);
					if constexpr (nmp) nmap_hit(a, nmap_args(acc_args...), bi, o, dir, n, ns, sm);
					if constexpr (tex) hA[depth] = tex_hit(a, tex_args(acc_args...), bi, o, dir);
					bool sl = false;                              // specular: this hit takes the mirror lobe
					float pm = 0.0f;
					float gi = 0.0f;                              // transparency: the triangle's ior; > 0: an interface, a specular hit
					if constexpr (gls) {
						gi = glass_table(acc_args...)[bi].w;
						if (gi > 0.0f) sl = true;
						else { pm = spec_table(acc_args...)[bi].w; sl = spec_lobe(a.seed, pixel, s0 + s, depth, pm); }
					} else if constexpr (spc) { pm = spec_table(acc_args...)[bi].w; sl = spec_lobe(a.seed, pixel, s0 + s, depth, pm); }
					if constexpr (mis) {
						f3 wd, Lc; float tm;
						const f3 x = add3(o, scale3(dir, bd));
						const float* m = a.mats + (size_t)bi * 6;
						const bool full = depth == 0 || (spc && (hidx[depth > 0 ? depth - 1 : 0] & kSpecBit) != 0);   // after a mirror bounce e_d counts in full
						const f3 De = full ? mk3(m[3], m[4], m[5]) : mis_emit(a, mis_tipdf(acc_args...), dir, bd, bi);
						f3 Ld = mk3(0.0f, 0.0f, 0.0f);
						// the light sample of a textured hit takes the hit's albedo.  Two copies of the block: the kernels without TexArgs keep
						// the lines, and so the instructions, they had before the element existed (tools/listing_diff.py)
						if constexpr (tex) {
							if (depth < kNeeDepths && !sl && nee_light<true, env, true>(a, nee_args(acc_args...), pixel, s0 + s, depth, x, ns, bi, wd, tm, Lc, env_map(acc_args...), &hA[depth]) && (!smo || smooth_light_ok(sm, wd, n))) {
								float sd; int si;
								scan_bvh(B, x, wd, bi, sd, si, nullptr, nullptr, tm, true);
								my_scans++;
								if (si < 0) Ld = Lc;
								Ld = scale3(Ld, 1.0f / (1.0f - pm));   // L_d wD
							}
						} else
						if (depth < kNeeDepths && !sl && nee_light<true, env>(a, nee_args(acc_args...), pixel, s0 + s, depth, x, ns, bi, wd, tm, Lc, env_map(acc_args...)) && (!smo || smooth_light_ok(sm, wd, n))) {
							float sd; int si;
							scan_bvh(B, x, wd, bi, sd, si, nullptr, nullptr, tm, true);
							my_scans++;
							if (si < 0) Ld = Lc;
							if constexpr (spc) Ld = scale3(Ld, 1.0f / (1.0f - pm));   // L_d wD
						}
						hD[depth] = depth < kNeeDepths ? add3(De, Ld) : De;
					} else if constexpr (nee) {
						f3 wd, Lc; float tm;
						const f3 x = add3(o, scale3(dir, bd));
						hL[depth] = mk3(0.0f, 0.0f, 0.0f);
						if (nee_light(a, nee_args(acc_args...), pixel, s0 + s, depth, x, n, bi, wd, tm, Lc)) {
							float sd; int si;
							scan_bvh(B, x, wd, bi, sd, si, nullptr, nullptr, tm, true);
							my_scans++;
							if (si < 0) hL[depth] = Lc;
						}
					}
					f3 nd;
					bool tr = false;                              // transparency: the bounce is a transmission
					if (gls && gi > 0.0f) { tr = glass_bounce(a, pixel, s0 + s, depth, bi, gi, dir, ns, sm, nd, ended); hcos[depth] = 0.0f; }
					else if (spc && sl) {
						nd = spec_reflect(dir, ns); hcos[depth] = 0.0f;
						if constexpr (smo) ended = sm && (!(dot3(dir, ns) < 0.0f) || dot3(nd, n) < 0.0f);
						if constexpr (glo) { const float al = rough_table(acc_args...)[bi]; if (al > 0.0f) gloss_hit(a, pixel, s0 + s, depth, al, dir, ns, n, sm, nd, hcos[depth], ended); }
					} else {
						double r1, r2;
						philox_uniforms(a.seed, pixel, s0 + s, (uint32_t)depth, &r1, &r2);
						nd = rand_unit_vec(ns, r1, r2);
						hcos[depth] = dot3(nd, ns);
						if constexpr (smo) ended = sm && dot3(nd, n) < 0.0f;
					}
					hidx[depth] = spc && sl ? bi | kSpecBit : bi;
					if constexpr (gls) if (tr) hidx[depth] |= kTransBit;
					o = add3(o, scale3(dir, bd));
					dir = nd;
					src = bi;
					nh = depth + 1;
					if constexpr (smo) if (ended) alive = false;
					if constexpr (glo && !smo) if (ended) alive = false;
				} else {
					if constexpr (env) Em = env_miss<mis>(env_args(acc_args...).env, dir, depth == 0 || (hidx[depth > 0 ? depth - 1 : 0] & kSpecBit) != 0);
					alive = false;
				}
			}
		}
		f3 rec = mk3(0.0f, 0.0f, 0.0f);
		if constexpr (env) rec = Em;
#pragma unroll
		for (int depth = 4; depth >= 0; --depth) {
			if (depth < nh) {
				const int id = spc ? hidx[depth] & hmask : hidx[depth];
				const float* m = a.mats + (size_t)id * 6;
				f3 brdf = scale3(mk3(m[0], m[1], m[2]), kInvPi);
				if constexpr (tex) brdf = scale3(hA[depth], kInvPi);
				f3 e = mk3(m[3], m[4], m[5]);
				if constexpr (mis) e = hD[depth];
				else if constexpr (nee) e = add3(depth == 0 ? e : mk3(0.0f, 0.0f, 0.0f), hL[depth < kNeeDepths ? depth : 0]);
				if constexpr (glo) rec = gloss_unwind(glass_table(acc_args...), spec_table(acc_args...), hidx[depth], e, brdf, rec, hcos[depth]);
				else if constexpr (gls) rec = glass_unwind(glass_table(acc_args...), spec_table(acc_args...), hidx[depth], e, brdf, rec, hcos[depth]);
				else if constexpr (spc) rec = spec_unwind(spec_table(acc_args...)[id], (hidx[depth] & kSpecBit) != 0, e, brdf, rec, hcos[depth]);
				else rec = add3(e, scale3(scale3(mul3(brdf, rec), hcos[depth]), kInvP));
			}
		}
		accum = add3(accum, rec);
		if constexpr (adapt) { const double y = lum_proxy(rec.x, rec.y, rec.z); s1 = s1 + y; s2 = s2 + y * y; }
	}
	if constexpr (adapt) {                            // the frame is resolved from sums and counts (k_adapt_resolve)
		const AdaptArgs& q = adapt_args(acc_args...);
		if (valid) {
			q.sum[(size_t)pk * 3 + 0] = accum.x; q.sum[(size_t)pk * 3 + 1] = accum.y; q.sum[(size_t)pk * 3 + 2] = accum.z;
			q.s12[(size_t)pk * 2] = s1; q.s12[(size_t)pk * 2 + 1] = s2;
		}
		wave_add_scans(a.scans, my_scans);
		return;
	}
	if constexpr (HasAccum<Acc...>::value) {
		const AccumArgs& q = accum_args(acc_args...);
		if (valid) { q.sum[(size_t)k * 3 + 0] = accum.x; q.sum[(size_t)k * 3 + 1] = accum.y; q.sum[(size_t)k * 3 + 2] = accum.z; }
	}
	accum = scale3(accum, a.inv_n);
	if (valid) {
		a.out_rgba[k] = clamped_rgba(accum);
		if (a.out_accum) { a.out_accum[(size_t)k * 3] = accum.x; a.out_accum[(size_t)k * 3 + 1] = accum.y; a.out_accum[(size_t)k * 3 + 2] = accum.z; }
	}
	wave_add_scans(a.scans, my_scans);
}

// test-only (sphip_selftest_bvh_walk): scan_bvh itself on caller rays, in either form, with the walk's own counts -- steps taken
// (reaching 4 * n_leaves + 64 means the belt-and-braces bound ended the walk) and leaves visited
__global__ void __launch_bounds__(256) k_selftest_bvh_walk(const float* __restrict__ rays, uint32_t n_rays, const BvhArgs B, const int* __restrict__ src_idx,
                                                           const float* __restrict__ tmax, int any_hit, int* __restrict__ out_idx, float* __restrict__ out_d,
                                                           uint32_t* __restrict__ out_steps, uint32_t* __restrict__ out_leaves) {
	const uint32_t k = blockIdx.x * 256u + threadIdx.x;
	if (k >= n_rays) return;
	const float* r = rays + (size_t)k * 6;
	float bd; int bi;
	uint32_t st = 0, lv = 0;                           // a shadow ray stopped by the big list never starts the walk
	scan_bvh<true>(B, mk3(r[0], r[1], r[2]), mk3(r[3], r[4], r[5]), src_idx ? src_idx[k] : -1, bd, bi, &st, &lv, tmax ? tmax[k] : kMaxDist, any_hit != 0);
	out_idx[k] = bi; out_d[k] = bd; out_steps[k] = st; out_leaves[k] = lv;
}

} // namespace sp
