// The path integrator's shared device code: the argument structs of the path kernels and the device functions that a path calls
// at a surface hit (shade_normal, nee_light, mis_emit, spec_lobe / spec_reflect / spec_unwind) and at a miss (env_miss), with the small pieces the kernels
// share around the integrator (load_ray, flat_px, clamped_rgba).
//
// k_pt (sp_kernels.h), k_accel (sp_bvh.h) and both branches of k_pt_filter (sp_scan_kernels.h) call these in the same sequence at a
// hit; the sequence itself is still written out in each of the four (DESIGN.md section 5.9 names its steps and says why).  A new
// material or estimator term gets its arithmetic here, once, and its call in each of the four.
#pragma once

#include "sp_device_math.h"

#include <type_traits>

namespace sp {

// scan record: 48 B = 3 x float4, produced by k_repack
//   q0 = v0.x v0.y v0.z e1.x   q1 = e1.y e1.z e2.x e2.y   q2 = e2.z 0 0 0
struct KArgs {
	const float*  rays;        // n_rays * 6
	const float4* scan;        // n_tris * 3
	const float*  tris;        // n_tris * 12 (normals live at +9)
	const float*  mats;        // n_tris * 6
	uint32_t*     out_rgba;    // n_rays
	float*        out_accum;   // n_rays * 3 or nullptr
	unsigned long long* scans; // device counter
	uint32_t n_rays, n_tris, n_samples, flags;
	uint64_t seed;
	uint64_t pixel_base, tile_px, tile_stride_px;
	float inv_n;               // float(1.0/n_samples), cpu_renderer.cpp:77
	// sample chunks (filter kernels): blockIdx = chunk * px_blocks + pixel block; every sample's radiance is written to
	// samp[(sample * 3 + c) * samp_stride + ray] and k_resolve adds them up in sample order.  n_chunks <= 1: off
	uint32_t n_chunks, px_blocks, samp_stride;
	float* samp;
	// primary-hit reuse of the two-stage kernels (flags & 0x100): closest hit of every ray of the launch, from a pre-pass
	// (k_hit_filter, one scan per PIXEL); k_pt_filter starts every sample of the pixel from it.  nullptr: off
	const int*   prim_idx;     // n_rays
	const float* prim_d;       // n_rays
};

// progressive accumulation (sphip_render_device_accum, sphip_accum_step): sample j of a launch is global sample
// sample_base + j (what keys the counter RNG), and the per-pixel f32 sum starts from sum[3k..3k+2] and is written back there
// raw, in place.  sample_base == 0: sum is not read (a fresh accumulation needs no cleared buffer).  inv_n is then
// float(1.0/(sample_base + n_samples)), so a run of steps ends in the image of one render of all their samples, bit for bit:
// the samples are added to the same f32 sum one at a time, in the same order.
// The path-tracing kernels take it as an optional trailing argument (a parameter pack of zero or one AccumArgs): without it a
// kernel is the same code as before the switch existed, which is what sphip_render launches.
struct AccumArgs {
	float* sum;                // n_rays * 3, AoS like out_accum
	uint32_t sample_base;
};

// adaptive sampling (sphip_accum_begin_adaptive, sp_adaptive.h): a progressive launch over the still-active pixels only.  Ray k
// of the launch is local pixel list[k]: the host gathers the active rays into a dense buffer in list order, so the ray reads
// (and the primary-hit pre-pass) are those of a plain launch, while list[k] keys the RNG (shard_pixel) and indexes the running
// sum and the statistics s12[2 list[k] + {0, 1}] = S1, S2 of the per-sample luminance proxy y (lum_proxy), added in sample
// order like the f32 sum, in double.  The launch writes no pixels: k_adapt_resolve turns sums and counts into the whole frame.
// wst: the two-stage kernels park S1, S2 of every work slot there (2 x n_work doubles), as they park the f32 accumulator.
struct AdaptArgs : AccumArgs {
	const uint32_t* list;      // n_rays local pixel indices, ascending
	double* s12;               // n_local * 2
	double* wst;               // 2 * n_work (two-stage kernels only)
};
// next-event estimation (SPHIP_FLAG_NEE): the scene's light table, built on the host once per scene.
// Emitter e of the table is triangle tri[e]; cdf is the running double sum of the weights A * Esum; ipdf = (float)(W / Esum).
// It rides as the LAST element of the trailing pack: k_pt<V, NeeArgs>, k_pt_filter<R, S, SCAN, AccumArgs, NeeArgs>, ...  L: the
// two-stage kernels park the direct light of depth d there, L[(d * 3 + c) * n_work + slot] (12 B per depth and slot).
struct NeeArgs {
	const double* cdf;         // n ascending
	const int*    tri;         // n emitter triangle indices, ascending
	const float*  ipdf;        // n
	uint32_t n;                // emitters of positive weight (0: no direct light)
	double W;                  // cdf[n - 1]
	float* L;                  // two-stage kernels only
};
constexpr int kNeeDepths = 4;                                    // light samples at hits 0..3; the 5th hit would carry nothing
constexpr float kShadowMargin = 1.0f - 0x1p-10f;                  // tmax = dist * (1 - 2^-10)
constexpr float kTwoOverPi = (float)(2.0 / kPi);                  // 2 pi x the reference's direction density (nee_light)
// multiple importance sampling (SPHIP_FLAG_MIS with SPHIP_FLAG_NEE): NeeArgs plus the light table's pdf by
// triangle, tipdf[i] = ipdf of triangle i's table entry, 0 for a triangle not in the table.  It rides in NeeArgs' place:
// k_pt<V, MisArgs>, k_pt_filter<R, S, SCAN, AccumArgs, MisArgs>, ...  L: the two-stage kernels park the folded direct term D_d of
// depths 0..4 there (15 floats per slot instead of 12).
struct MisArgs : NeeArgs {
	const float* tipdf;        // n_tris
};
constexpr int kMisDepths = 5;                                     // MIS traces the 5th hit again: its emission counts
constexpr float kTwoPi = (float)(2.0 * kPi);
constexpr float kPiSq = (float)(kPi * kPi);

// ---- view::camera::get_viewport (view.h:94-132) on the device: one thread per pixel.
// The eight step constants are computed on the host in the reference's mixed double/float way (view.h:101-108).
struct ViewArgs {
	float x_max, x_step, h_x_step, y_max, y_step, h_y_step;
	float focal, cos_y, sin_y, cos_x, sin_x;
	float px, py, pz;
	uint32_t res_x, res_y;
	// which pixels: ray k of the output is global pixel pixel_base + (k / tile_px) * tile_stride_px + k % tile_px (sphip_shard);
	// the whole image is {0, res_x*res_y, 0} with n_local = res_x*res_y
	uint64_t pixel_base, tile_px, tile_stride_px;
	uint32_t n_local;
};
// per-sample camera rays (SPHIP_FLAG_CAMERA_SAMPLES): the viewport constants (the shard fields unused: the
// kernels key the ray by the global pixel they already know) and the lens.  It rides as the LAST element of the trailing pack:
// k_pt<V, CamArgs>, k_pt_filter<R, S, SCAN, AccumArgs, NeeArgs, CamArgs>, ...  Every sample's primary ray is then generated from
// (seed, global pixel, global sample) instead of being read from KArgs::rays.
struct CamArgs {
	ViewArgs v;
	float aperture;            // lens radius on the image plane, 0 = pinhole
	float focus_dist;          // local z of the plane in focus (aperture > 0)
};

// specular reflection (SPHIP_FLAG_SPECULAR, include/spath_hip.h): the scene's specular table, one float4 per
// triangle: ks.r ks.g ks.b p.  It rides between the estimator and the camera: k_pt<V, MisArgs, SpecArgs, CamArgs>, ...  A hit of
// depth d takes the mirror lobe iff the first uniform of Philox stream kSpecStream + d is below p; the path history marks such a
// hit with kSpecBit in its triangle index (triangle indices stay below 2^30: sphip_set_specular checks it).
struct SpecArgs {
	const float4* spec;        // n_tris
};
constexpr uint32_t kSpecStream = 32u;
constexpr int kSpecBit = 0x40000000;

// transparency (SPHIP_FLAG_DIELECTRIC, include/spath_hip.h): the scene's dielectric table, one float4 per
// triangle: kt.r kt.g kt.b ior; ior = 0 leaves the triangle what it is.  It rides IN SpecArgs' PLACE (as MisArgs rides in NeeArgs'):
// k_pt<V, MisArgs, GlassArgs, NormArgs, CamArgs>, ...; spec is the scene's specular table, or a table of zeros when
// SPHIP_FLAG_SPECULAR is not set (p = 0, wD = 1.0f: the diffuse arithmetic's bits).  A hit on a dielectric triangle is a specular
// hit (kSpecBit) whose lobe is drawn from the same stream kSpecStream + d against the Fresnel reflectance; a transmitted bounce
// carries kTransBit as well (triangle indices stay below 2^29: sphip_set_dielectric checks it).
struct GlassArgs : SpecArgs {
	const float4* glass;       // n_tris
};
constexpr int kTransBit = 0x20000000;

// the context's map as the device functions see it.  rc[j * n + i]: the running double sum of wt along row j; marg[j]: the running
// double sum of rc[j][n - 1]; T = marg[n - 1]; tpdf: the scene-dependent density per texel (0 everywhere until a light table is built)
struct EnvMap {
	const float*  texels;      // n * n * 3, texel (i, j) at (j * n + i) * 3
	const double* rc;          // n * n
	const double* marg;        // n
	const float*  tpdf;        // n * n
	double T;
	uint32_t n;
};
constexpr uint32_t kEnvMaxN = 2048;

// environment lighting (SPHIP_FLAG_ENVIRONMENT, include/spath_hip.h): the map and its tables beside the tables of
// GlassArgs, IN GlassArgs' PLACE (as GlassArgs rides in SpecArgs'): k_pt<V, MisArgs, EnvArgs, NormArgs, CamArgs>, ...  spec and glass are the
// scene's tables, or tables of zeros when SPHIP_FLAG_SPECULAR or SPHIP_FLAG_DIELECTRIC is not set (p = 0, ior = 0: the diffuse
// arithmetic's bits).  With MisArgs the light table of the NeeArgs fields is the flagged one: its last entry, tri = -1, is the map.
// M: the two-stage kernels park the miss term of a path there, M[c * n_work + slot]
struct EnvArgs : GlassArgs {
	EnvMap env;
	float* M;                  // two-stage kernels only
};
constexpr uint32_t kEnvStream = 40u;

// glossy reflection (SPHIP_FLAG_GLOSSY, include/spath_hip.h): the scene's roughness table, one float per triangle:
// the GGX alpha of the triangle's mirror lobe; alpha = 0 leaves the mirror what it is.  It rides IN EnvArgs' PLACE (as EnvArgs rides in
// GlassArgs'): k_pt<V, MisArgs, GlossArgs, NormArgs, CamArgs>, ...  glass is the scene's table or zeros as in EnvArgs; env is the context's
// map, or its 1 x 1 black map (T = 0: no entry in the light table, every miss carries 0) when SPHIP_FLAG_ENVIRONMENT is not set.  A
// glossy hit is a specular hit (kSpecBit) whose weight g rides in the history's cosine slot, which is 0 for every other specular hit
struct GlossArgs : EnvArgs {
	const float* rough;        // n_tris
};
constexpr uint32_t kGlossStream = 48u;

// textures (SPHIP_FLAG_TEXTURE, include/spath_hip.h): the scene's UV table, 6 floats per triangle: s0 t0 s1 t1 s2 t2
// for v0 v1 v2 (a row of zeros leaves its triangle untextured), and the context's atlas, tw x th RGB texels, texel (i, j) at
// (j * tw + i) * 3.  It rides IN GlossArgs' PLACE (as GlossArgs rides in EnvArgs'): k_pt<V, MisArgs, TexArgs, NormArgs, CamArgs>, ...
// spec, glass and rough are the scene's tables or zeros, env the context's map or its black one, as in GlossArgs.  The hit's albedo
// rho * c (tex_albedo) replaces the material's reflectance in the unwind's brdf and in the light sample, nowhere else.
// A: the two-stage kernels park the albedo of depth d there, A[(d * 3 + c) * n_work + slot] (12 B per depth and slot)
struct TexArgs : GlossArgs {
	const float* uv;           // n_tris * 6
	const float* atlas;        // tw * th * 3
	uint32_t tw, th;
	float* A;                  // two-stage kernels only
};
constexpr uint32_t kTexMaxN = 4096;

// normal mapping (SPHIP_FLAG_NORMAL_MAP, include/spath_hip.h): the context's normal map, nw x nh RGB texels holding a
// tangent-space vector (x, y, z) as signed floats, texel (i, j) at (j * nw + i) * 3, addressed by the UV table of TexArgs.  It rides IN
// TexArgs' PLACE (as TexArgs rides in GlossArgs'), and ALWAYS with a NormArgs behind it: k_pt<V, MisArgs, NmapArgs, NormArgs, CamArgs>, ...
// Without SPHIP_FLAG_TEXTURE the atlas is the context's 1 x 1 white texel (rho * 1.0f = rho), without SPHIP_FLAG_SMOOTH the vertex normals
// are a table of zeros (every triangle flat); the other tables as in TexArgs.  Each hit's shading normal is replaced by the map's normal
// in the hit's tangent frame (nmap_normal), and the hit is then a smooth one in every rule.  Nothing is parked per depth
struct NmapArgs : TexArgs {
	const float* nmap;         // nw * nh * 3
	uint32_t nw, nh;
};

// smooth shading (SPHIP_FLAG_SMOOTH, include/spath_hip.h): the scene's vertex normals, 9 floats per triangle:
// n0.xyz n1.xyz n2.xyz for v0 v1 v2.  It rides after the specular table, before the camera: k_pt<V, MisArgs, SpecArgs, NormArgs,
// CamArgs>, ...  Every hit shades with the interpolated normal of shade_normal; a row of zeros leaves its triangle flat.
struct NormArgs {
	const float* vnorm;        // n_tris * 9
};

// the pack's optional elements, found by type wherever they sit (MisArgs is a NeeArgs, AdaptArgs an AccumArgs)
template <typename T, typename... P> struct PackHas { static constexpr bool value = (std::is_same<T, P>::value || ...); };
template <typename... Acc> struct IsAdapt { static constexpr bool value = PackHas<AdaptArgs, Acc...>::value; };
template <typename... Acc> struct IsMis { static constexpr bool value = PackHas<MisArgs, Acc...>::value; };
template <typename... Acc> struct IsNee { static constexpr bool value = PackHas<NeeArgs, Acc...>::value || IsMis<Acc...>::value; };
template <typename... Acc> struct IsCam { static constexpr bool value = PackHas<CamArgs, Acc...>::value; };
template <typename... Acc> struct IsNmap { static constexpr bool value = PackHas<NmapArgs, Acc...>::value; };
template <typename... Acc> struct IsTex { static constexpr bool value = PackHas<TexArgs, Acc...>::value || IsNmap<Acc...>::value; };
template <typename... Acc> struct IsGloss { static constexpr bool value = PackHas<GlossArgs, Acc...>::value || IsTex<Acc...>::value; };
template <typename... Acc> struct IsEnv { static constexpr bool value = PackHas<EnvArgs, Acc...>::value || IsGloss<Acc...>::value; };
template <typename... Acc> struct IsGlass { static constexpr bool value = PackHas<GlassArgs, Acc...>::value || IsEnv<Acc...>::value; };
template <typename... Acc> struct IsSpec { static constexpr bool value = PackHas<SpecArgs, Acc...>::value || IsGlass<Acc...>::value; };
// what clears the marks of the path history from a triangle index
template <typename... Acc> struct HistMask { static constexpr int value = IsGlass<Acc...>::value ? ~(kSpecBit | kTransBit) : ~kSpecBit; };
template <typename... Acc> struct IsNorm { static constexpr bool value = PackHas<NormArgs, Acc...>::value; };
// a running sum rides in the pack (progressive or adaptive)
template <typename... Acc> struct HasAccum { static constexpr bool value = PackHas<AccumArgs, Acc...>::value || IsAdapt<Acc...>::value; };
// the first element of the pack that is a T
template <typename T, typename H, typename... R>
SP_DEV const T& pack_get(const H& h, const R&... r) {
	if constexpr (std::is_base_of<T, H>::value) return h;
	else return pack_get<T>(r...);
}
template <typename... P> SP_DEV const AdaptArgs& adapt_args(const P&... p) { return pack_get<AdaptArgs>(p...); }
template <typename... P> SP_DEV const AccumArgs& accum_args(const P&... p) { return pack_get<AccumArgs>(p...); }
template <typename... P> SP_DEV const NeeArgs& nee_args(const P&... p) { return pack_get<NeeArgs>(p...); }
template <typename... P> SP_DEV const CamArgs& cam_args(const P&... p) { return pack_get<CamArgs>(p...); }
template <typename... P> SP_DEV const float4* spec_table(const P&... p) { return pack_get<SpecArgs>(p...).spec; }
template <typename... P> SP_DEV const float4* glass_table(const P&... p) { return pack_get<GlassArgs>(p...).glass; }
template <typename... P> SP_DEV const EnvArgs& env_args(const P&... p) { return pack_get<EnvArgs>(p...); }
// the map of the pack for nee_light, nullptr without one
template <typename... P> SP_DEV const EnvMap* env_map(const P&... p) {
	if constexpr (IsEnv<P...>::value) return &pack_get<EnvArgs>(p...).env;
	else return nullptr;
}
template <typename... P> SP_DEV const float* rough_table(const P&... p) { return pack_get<GlossArgs>(p...).rough; }
template <typename... P> SP_DEV const TexArgs& tex_args(const P&... p) { return pack_get<TexArgs>(p...); }
template <typename... P> SP_DEV const NmapArgs& nmap_args(const P&... p) { return pack_get<NmapArgs>(p...); }
template <typename... P> SP_DEV const float* norm_table(const P&... p) { return pack_get<NormArgs>(p...).vnorm; }
template <typename... P> SP_DEV const float* mis_tipdf(const P&... p) { return pack_get<MisArgs>(p...).tipdf; }
// local pixel of launch ray k (k < n_rays): k itself, or the active list's entry
template <typename... Acc>
SP_DEV uint32_t local_px(uint32_t k, const Acc&... acc_args) {
	if constexpr (IsAdapt<Acc...>::value) return adapt_args(acc_args...).list[k];
	else return k;
}
// the per-sample luminance proxy of the convergence rule: ((double)r + (double)g) + (double)b of the sample's f32 radiance
SP_DEV double lum_proxy(float r, float g, float b) { return ((double)r + (double)g) + (double)b; }

// ---- smooth shading (include/spath_hip.h): the shading normal ns of the hit of ray (o, dir) on the triangle
// whose vertices are tv[0..8] (v0 v1 v2) and whose vertex normals are vn[0..8]; n is the triangle's stored normal turned against dir.
//   bary:    u, v exactly as ray_tri_strict computed them for this triangle (geom.h:200-212), once, for the winning triangle
//   interp:  w = (1 - u) - v;  m = (n0 w + n1 u) + n2 v;  l2 = dot3(m, m);  smooth iff l2 > 0 and finite
//            ns = m / sqrtf(l2) per component, turned to n's side; otherwise ns = n and the hit is the flat one
// Returns whether the hit is smooth.  uv: where the selftest wants u, v.
// The light sample of a smooth hit (nee_light with ns for n) counts only when its direction is above the stored normal as well
// (smooth_light_ok): both strategies of MIS then integrate over {w . ns > 0, w . n > 0}.
SP_DEV bool shade_normal(const float* __restrict__ tv, const float* __restrict__ vn, f3 o, f3 dir, f3 n, f3& ns, float* uv = nullptr) {
	const f3 v0 = mk3(tv[0], tv[1], tv[2]);
	const f3 e1 = sub3(mk3(tv[3], tv[4], tv[5]), v0), e2 = sub3(mk3(tv[6], tv[7], tv[8]), v0);   // geom.h:200-201
	const f3 h = cross3(dir, e2);                    // :202
	const float a = dot3(e1, h);                     // :203
	const float f = recip_ieee(a);                   // :206
	const f3 s = sub3(o, v0);                        // :207
	const float u = f * dot3(s, h);                  // :208
	const f3 q = cross3(s, e1);                      // :211
	const float v = f * dot3(dir, q);                // :212
	if (uv) { uv[0] = u; uv[1] = v; }
	const float w = (1.0f - u) - v;
	const f3 m = add3(add3(scale3(mk3(vn[0], vn[1], vn[2]), w), scale3(mk3(vn[3], vn[4], vn[5]), u)), scale3(mk3(vn[6], vn[7], vn[8]), v));
	const float l2 = dot3(m, m);
	const bool sm = l2 > 0.0f && l2 < __builtin_inff();
	ns = n;
	if (sm) {
		const float l = __builtin_sqrtf(l2);
		ns = mk3(m.x / l, m.y / l, m.z / l);
		if (dot3(ns, n) < 0.0f) ns = scale3(ns, -1.0f);
	}
	return sm;
}

SP_DEV bool smooth_light_ok(bool sm, f3 wd, f3 n) { return !sm || dot3(wd, n) > 0.0f; }

// ---- MIS (include/spath_hip.h): u = p_l / q, the light table's density over the reference's BSDF density,
// both per solid angle, for a direction w that reaches emitter j at distance sqrt(dist2) under cos_y.  A NaN quotient (0/0 or
// inf/inf) counts as 0, so 1 / (1 + u) is a weight in [0, 1] for every input.
SP_DEV float mis_u(float sxz, float dist2, float cos_y, float ipdf) {
	const float u = ((kPiSq * sxz) * dist2) / (cos_y * ipdf);
	return u == u ? u : 0.0f;
}
// the emission e_d of the triangle bi that the BSDF direction dir found at distance bd (d >= 1), weighted by the balance heuristic:
// e_d / (1 + u_b), or e_d itself when bi is not in the light table (tipdf[bi] = 0: the light sample never picks it)
SP_DEV f3 mis_emit(const KArgs& a, const float* tipdf, f3 dir, float bd, int bi) {
	const float* m = a.mats + (size_t)bi * 6;
	const f3 e = mk3(m[3], m[4], m[5]);
	const float ip = tipdf[bi];
	if (!(ip > 0.0f)) return e;
	const float* tn = a.tris + (size_t)bi * 12 + 9;
	const float cos_y = fabsf(dot3(dir, mk3(tn[0], tn[1], tn[2])));
	const float sxz = __builtin_sqrtf(dir.x * dir.x + dir.z * dir.z);
	const float opu = 1.0f + mis_u(sxz, bd * bd, cos_y, ip);
	return mk3(e.x / opu, e.y / opu, e.z / opu);
}

// ---- environment lighting (include/spath_hip.h "environment lighting").  Both mappings need only + - * /,
// fabsf, sqrtf and selects, so the numpy model (tests/env_model.py) restates them bit for bit.
SP_DEV float env_sgn(float t) { return t < 0.0f ? -1.0f : 1.0f; }
SP_DEV uint32_t env_cell(float a, uint32_t n) {
	const int i = (int)((a * 0.5f + 0.5f) * (float)n);
	return i < 0 ? 0u : i > (int)n - 1 ? n - 1u : (uint32_t)i;
}

// the texel that direction d sees (any scale of d), and r3 = |p|^3 for p = d / (|d.x| + |d.y| + |d.z|): da db = r3 d omega, so a density
// per unit (a, b) area times r3 is one per solid angle.
// Returns whether there is a texel: not for a zero, an infinite or a NaN direction
SP_DEV bool env_lookup(f3 d, uint32_t n, uint32_t& i, uint32_t& j, float& r3) {
	const float s = (fabsf(d.x) + fabsf(d.y)) + fabsf(d.z);
	i = 0; j = 0; r3 = 0.0f;
	if (!(s > 0.0f) || !(s < __builtin_inff())) return false;
	const f3 p = mk3(d.x / s, d.y / s, d.z / s);
	float a = p.x, b = p.z;
	if (!(p.y >= 0.0f)) {                                          // the lower half, folded outwards over the square's diagonals
		a = (1.0f - fabsf(p.z)) * env_sgn(p.x);
		b = (1.0f - fabsf(p.x)) * env_sgn(p.z);
	}
	i = env_cell(a, n);
	j = env_cell(b, n);
	const float l2 = dot3(p, p);
	r3 = __builtin_sqrtf(l2) * l2;
	return true;
}

// the first k in [0, m) with t[k] > x, m - 1 when there is none (t ascending)
SP_DEV uint32_t env_first_above(const double* __restrict__ t, uint32_t m, double x) {
	uint32_t lo = 0, hi = m - 1u;
	while (lo < hi) {
		const uint32_t mid = (lo + hi) >> 1;
		if (t[mid] > x) hi = mid; else lo = mid + 1u;
	}
	return lo;
}

// one draw from the map's tables: (r8, r9) pick the texel (row by marg, column by the row's rc), (r3u, r4u) the place in it.
// wd: the unit direction of that place; r3 = |g|^3 of the octahedron point g it came from
SP_DEV void env_sample(const EnvMap& e, double r8, double r9, double r3u, double r4u, uint32_t& i, uint32_t& j, f3& wd, float& r3) {
	j = env_first_above(e.marg, e.n, r8 * e.T);
	const double* row = e.rc + (size_t)j * e.n;
	i = env_first_above(row, e.n, r9 * row[e.n - 1u]);
	const float step = 2.0f / (float)e.n;
	const float a = ((float)i + (float)r3u) * step - 1.0f;
	const float b = ((float)j + (float)r4u) * step - 1.0f;
	const float y = (1.0f - fabsf(a)) - fabsf(b);
	float x = a, z = b;
	if (!(y >= 0.0f)) {
		x = (1.0f - fabsf(b)) * env_sgn(a);
		z = (1.0f - fabsf(a)) * env_sgn(b);
	}
	const f3 g = mk3(x, y, z);
	const float l2 = dot3(g, g);
	const float l = __builtin_sqrtf(l2);
	wd = mk3(g.x / l, g.y / l, g.z / l);
	r3 = l * l2;
}


// the balance ratio of a direction of texel density tp (per unit (a, b) area) against the BSDF density q = 1 / (pi^2 sxz):
// ((pi^2 sxz) r3) tp, 0 where that is NaN
SP_DEV float env_u(float sxz, float r3, float tp) {
	const float u = ((kPiSq * sxz) * r3) * tp;
	return u == u ? u : 0.0f;
}
// what the ray of direction dir that left the scene carries: the texel's radiance, under MIS (and unless full: the camera's ray, or
// the ray after a specular or transmitted bounce) weighted by 1 / (1 + u_env) where the light sample can draw the texel
template <bool MIS>
SP_DEV f3 env_miss(const EnvMap& e, f3 dir, bool full) {
	uint32_t i, j;
	float r3;
	if (!env_lookup(dir, e.n, i, j, r3)) return mk3(0.0f, 0.0f, 0.0f);
	const size_t t = (size_t)j * e.n + i;
	const f3 Le = mk3(e.texels[t * 3], e.texels[t * 3 + 1], e.texels[t * 3 + 2]);
	if constexpr (!MIS) return Le;
	const float tp = e.tpdf[t];
	if (full || !(tp > 0.0f)) return Le;
	const float opu = 1.0f + env_u(__builtin_sqrtf(dir.x * dir.x + dir.z * dir.z), r3, tp);
	return mk3(Le.x / opu, Le.y / opu, Le.z / opu);
}
// the light sample that picked the map's entry of the light table, at a hit on triangle src of shading normal n: (r3u, r4u) are the
// uniforms of stream 8 + d that place a triangle sample.  The shadow ray (x, wd) is unbounded: anything it hits occludes.
// TEX: the hit's reflectance is *refl, not the material's (textures: tex_albedo)
template <bool TEX = false>
SP_DEV bool env_light(const KArgs& a, const EnvMap& e, uint32_t pixel, uint32_t sample, int depth, f3 n, int src, double r3u, double r4u,
                      f3& wd, float& tmax, f3& L, const f3* refl = nullptr) {
	double r8, r9;
	philox_uniforms(a.seed, pixel, sample, kEnvStream + (uint32_t)depth, &r8, &r9);
	uint32_t i, j;
	float r3;
	env_sample(e, r8, r9, r3u, r4u, i, j, wd, r3);
	const float cos_x = dot3(wd, n);
	if (!(cos_x > 0.0f)) return false;
	const size_t t = (size_t)j * e.n + i;
	const float sxz = __builtin_sqrtf(wd.x * wd.x + wd.z * wd.z);
	const float g = (kTwoPi * cos_x) / (1.0f + env_u(sxz, r3, e.tpdf[t]));
	tmax = kMaxDist;
	const float* ms = a.mats + (size_t)src * 6;
	if constexpr (TEX) L = mul3(scale3(*refl, kInvPi), scale3(mk3(e.texels[t * 3], e.texels[t * 3 + 1], e.texels[t * 3 + 2]), g));
	else L = mul3(scale3(mk3(ms[0], ms[1], ms[2]), kInvPi), scale3(mk3(e.texels[t * 3], e.texels[t * 3 + 1], e.texels[t * 3 + 2]), g));
	return true;
}

// ---- next-event estimation: one light sample at the hit x of a path (include/spath_hip.h).
// n: the hit triangle's normal as the path uses it (turned against the incoming ray); src: the hit triangle.  Returns whether a
// shadow ray (x, wd) with the bound tmax is to be traced, and then L = the direct light it carries when nothing occludes it.
// MIS: L carries the balance heuristic's weight u / (1 + u), and sxz = 0 is no early-out (L is finite).
// ENV: the table is the flagged one, whose entry of triangle -1 is the environment map *em (env_light).
// TEX: the hit's reflectance is *refl, not the material's (textures: tex_albedo)
template <bool MIS = false, bool ENV = false, bool TEX = false>
SP_DEV bool nee_light(const KArgs& a, const NeeArgs& ne, uint32_t pixel, uint32_t sample, int depth, f3 x, f3 n, int src,
                      f3& wd, float& tmax, f3& L, const EnvMap* em = nullptr, const f3* refl = nullptr) {
	if (ne.n == 0) return false;
	double r3, r4, r5, r6;
	philox_uniforms(a.seed, pixel, sample, 8u + (uint32_t)depth, &r3, &r4);
	philox_uniforms(a.seed, pixel, sample, 16u + (uint32_t)depth, &r5, &r6);
	// the first emitter whose cdf exceeds r5 W, the last one when rounding leaves none
	const double t = r5 * ne.W;
	uint32_t lo = 0, hi = ne.n - 1u;
	while (lo < hi) {
		const uint32_t mid = (lo + hi) >> 1;
		if (ne.cdf[mid] > t) hi = mid; else lo = mid + 1u;
	}
	const int li = ne.tri[lo];
	if (li == src) return false;
	if constexpr (ENV) if (li < 0) return env_light<TEX>(a, *em, pixel, sample, depth, n, src, r3, r4, wd, tmax, L, refl);
	const float* tv = a.tris + (size_t)li * 12;
	const f3 v0 = mk3(tv[0], tv[1], tv[2]);
	const f3 e1 = sub3(mk3(tv[3], tv[4], tv[5]), v0), e2 = sub3(mk3(tv[6], tv[7], tv[8]), v0);
	const float ua = (float)__builtin_sqrt(r3), ub = (float)r4;
	const f3 y = add3(add3(v0, scale3(e1, ua * (1.0f - ub))), scale3(e2, ua * ub));
	const f3 w = sub3(y, x);
	const float dist2 = dot3(w, w);
	if (!(dist2 > 0.0f)) return false;
	const float dist = __builtin_sqrtf(dist2);
	wd = mk3(w.x / dist, w.y / dist, w.z / dist);
	const float cos_x = dot3(wd, n);
	const float cos_y = fabsf(dot3(wd, mk3(tv[9], tv[10], tv[11])));      // emitters are two-sided
	// the reference's direction sampler (rand_unit_vec, geom.h:164-177) draws the elevation from the world y plane uniformly in ANGLE:
	// density q = 1 / (pi^2 sqrt(x^2 + z^2)) per solid angle, while the path weight assumes 1/p = 2 pi.  The plain estimator's
	// expectation therefore carries 2 pi q(w) per bounce; the light sample carries the same factor, 2 / (pi sxz), so that both
	// estimate the same image
	const float sxz = __builtin_sqrtf(wd.x * wd.x + wd.z * wd.z);
	if constexpr (MIS) {
		if (!(cos_x > 0.0f) || !(cos_y > 0.0f)) return false;
	} else {
		if (!(cos_x > 0.0f) || !(cos_y > 0.0f) || !(sxz > 0.0f)) return false;
	}
	tmax = dist * kShadowMargin;
	const float* me = a.mats + (size_t)li * 6;
	const float* ms = a.mats + (size_t)src * 6;
	float g;
	// MIS: g (u / (1 + u)) with u = ((pi^2 sxz) dist2) / (cos_y ipdf): the 1 / dist2 and 1 / sxz factors cancel, g <= 2 pi
	if constexpr (MIS) g = (kTwoPi * cos_x) / (1.0f + mis_u(sxz, dist2, cos_y, ne.ipdf[lo]));
	else g = (((cos_x * cos_y) / dist2) * ne.ipdf[lo]) * (kTwoOverPi / sxz);
	if constexpr (TEX) L = mul3(scale3(*refl, kInvPi), scale3(mk3(me[3], me[4], me[5]), g));
	else L = mul3(scale3(mk3(ms[0], ms[1], ms[2]), kInvPi), scale3(mk3(me[3], me[4], me[5]), g));
	return true;
}

// ---- specular reflection (include/spath_hip.h).  The lobe of the hit of depth d on a triangle of mirror
// probability p: specular iff r7 < (double)p, r7 the first uniform of stream kSpecStream + d
SP_DEV bool spec_lobe(uint64_t seed, uint32_t pixel, uint32_t sample, int depth, float p) {
	double r7, r8;
	philox_uniforms(seed, pixel, sample, kSpecStream + (uint32_t)depth, &r7, &r8);
	return r7 < (double)p;
}
// the mirror direction of dir about n: dir - n * (c + c), c = dot3(dir, n); not renormalised
SP_DEV f3 spec_reflect(f3 dir, f3 n) {
	const float c = dot3(dir, n);
	return sub3(dir, scale3(n, c + c));
}
// one step of the unwind at a hit on triangle id whose lobe was specular (sl) or diffuse: E + ((ks * rec) * (1 / p)), or today's
// expression scaled once more, by 1 / (1 - p)
SP_DEV f3 spec_unwind(const float4 q, bool sl, f3 e, f3 brdf, f3 rec, float ct) {
	if (sl) return add3(e, scale3(mul3(mk3(q.x, q.y, q.z), rec), 1.0f / q.w));
	return add3(e, scale3(scale3(scale3(mul3(brdf, rec), ct), kInvP), 1.0f / (1.0f - q.w)));
}

// ---- transparency (include/spath_hip.h "transparency"): Snell and Fresnel at a smooth interface of index ior
// for the ray dir and the shading normal ns (turned against dir); entering: the ray comes from the vacuum side.  f32, every operation
// rounded on its own.  Fr: the unpolarised reflectance; tir: total internal reflection (Fr and nt then mean nothing); nt: the
// refracted direction, not renormalised; c = dot3(dir, ns)
SP_DEV void dielectric(f3 dir, f3 ns, float ior, bool entering, float& Fr, bool& tir, f3& nt, float& c) {
	const float eta = entering ? 1.0f / ior : ior;
	c = dot3(dir, ns);
	const float ci = -c;
	const float k = 1.0f - (eta * eta) * (1.0f - ci * ci);
	tir = !(k > 0.0f);
	const float ct = __builtin_sqrtf(k);
	const float a = eta * ci, b = eta * ct;
	const float rs = (a - ct) / (a + ct), rp = (ci - b) / (ci + b);
	Fr = 0.5f * (rs * rs + rp * rp);
	nt = add3(scale3(dir, eta), scale3(ns, a - ct));
}
// the bounce of the hit of depth d on dielectric triangle bi (ior > 0): the lobe is drawn from the specular lobe's stream (that
// lobe is not drawn on such a triangle), transmit iff !tir and (double)Fr <= r7 (a NaN Fr reflects).  sm: the hit is smooth
// (shade_normal); the path then ends when dir is not against ns, when a reflection goes below the stored normal (the mirror's rule)
// or when a transmission stays above it.  Returns whether the bounce is a transmission
SP_DEV bool glass_bounce(const KArgs& a, uint32_t pixel, uint32_t sample, int depth, int bi, float ior, f3 dir, f3 ns, bool sm, f3& nd, bool& ended) {
	const float* tn = a.tris + (size_t)bi * 12 + 9;
	f3 n = mk3(tn[0], tn[1], tn[2]);
	const bool entering = !(dot3(n, dir) > 0.0f);
	if (!entering) n = scale3(n, -1.0f);
	float Fr, c;
	bool tir;
	f3 nt;
	dielectric(dir, ns, ior, entering, Fr, tir, nt, c);
	double r7, r8;
	philox_uniforms(a.seed, pixel, sample, kSpecStream + (uint32_t)depth, &r7, &r8);
	const bool tr = !tir && (double)Fr <= r7;
	nd = tr ? nt : spec_reflect(dir, ns);
	const bool below = dot3(nd, n) < 0.0f;
	ended = sm && (!(c < 0.0f) || (tr ? !below : below));
	return tr;
}
// one step of the unwind with a dielectric table: E + rec after a reflection at an interface, E + kt * rec after a transmission,
// spec_unwind's step at every other triangle.  id: the history's index with its marks
SP_DEV f3 glass_unwind(const float4* __restrict__ glass, const float4* __restrict__ spec, int id, f3 e, f3 brdf, f3 rec, float ct) {
	const int i = id & ~(kSpecBit | kTransBit);
	const float4 g = glass[i];
	if (g.w > 0.0f) return (id & kTransBit) ? add3(e, mul3(mk3(g.x, g.y, g.z), rec)) : add3(e, rec);
	return spec_unwind(spec[i], (id & kSpecBit) != 0, e, brdf, rec, ct);
}

// ---- glossy reflection (include/spath_hip.h "glossy reflection"): one draw from the GGX distribution of visible
// normals (Heitz 2018) of roughness al > 0 around the shading normal ns (turned against dir), for the uniforms (u1, u2).  f32, every
// operation rounded on its own, but the disk's radius (a double sqrt) and its angle (double, as the lens).  m: the microfacet normal;
// nd: dir mirrored about m, not renormalised; g: the separable Smith term G1 of nd, the sample's whole weight beside ks / p.
// Returns ok: nd is above ns (otherwise the path ends at this hit and g means nothing)
SP_DEV bool gloss_bounce(f3 dir, f3 ns, float al, double u1, double u2, f3& m, f3& nd, float& g) {
	const float c = dot3(dir, ns);
	// frame: a branchless orthonormal basis (t, bt, ns)
	const float sg = ns.z < 0.0f ? -1.0f : 1.0f;
	const float a = -1.0f / (sg + ns.z);
	const float b = (ns.x * ns.y) * a;
	const f3 t = mk3(1.0f + (sg * (ns.x * ns.x)) * a, sg * b, (-sg) * ns.x);
	const f3 bt = mk3(b, sg + (ns.y * ns.y) * a, -ns.y);
	// view: the direction back along the ray in that frame, stretched to the unit-roughness configuration
	const f3 v = mk3(-dot3(dir, t), -dot3(dir, bt), -c);
	const f3 h = mk3(al * v.x, al * v.y, v.z);
	const float hl = __builtin_sqrtf(dot3(h, h));
	const f3 vh = mk3(h.x / hl, h.y / hl, h.z / hl);
	// basis: orthogonal to vh
	const float l2 = vh.x * vh.x + vh.y * vh.y;
	f3 T1 = mk3(1.0f, 0.0f, 0.0f);
	if (l2 > 0.0f) { const float l = __builtin_sqrtf(l2); T1 = mk3(-vh.y / l, vh.x / l, 0.0f); }
	const f3 T2 = cross3(vh, T1);
	// disk: a uniform point of the unit disk, warped onto the projection of the visible half
	const float r = (float)__builtin_sqrt(u1);
	const float phi = (float)((u2 * kPi) * 2.0);
	float sn, cs;
	sincos_glibc(phi, &sn, &cs);
	const float p1 = r * cs;
	float p2 = r * sn;
	const float s = 0.5f * (1.0f + vh.z);
	float q = 1.0f - p1 * p1;
	q = q > 0.0f ? q : 0.0f;
	p2 = (1.0f - s) * __builtin_sqrtf(q) + s * p2;
	const float z2 = (1.0f - p1 * p1) - p2 * p2;
	const float z = __builtin_sqrtf(z2 > 0.0f ? z2 : 0.0f);
	const f3 nh = add3(add3(scale3(T1, p1), scale3(T2, p2)), scale3(vh, z));
	// normal: unstretched, back in the world
	const f3 ne = mk3(al * nh.x, al * nh.y, nh.z > 0.0f ? nh.z : 0.0f);
	const float nl = __builtin_sqrtf(dot3(ne, ne));
	const f3 ml = mk3(ne.x / nl, ne.y / nl, ne.z / nl);
	m = add3(add3(scale3(t, ml.x), scale3(bt, ml.y)), scale3(ns, ml.z));
	nd = spec_reflect(dir, m);
	// weight: cl stands for the cosine although nd has dir's length
	const float cl = dot3(nd, ns);
	g = (cl + cl) / (cl + __builtin_sqrtf(al * al + (1.0f - al * al) * (cl * cl)));
	g = g > 1.0f ? 1.0f : g;                           // a dir a rounding longer than unit gives cl, and so g, a rounding above 1
	return cl > 0.0f;
}
// the bounce of the hit of depth d that took the mirror lobe of a triangle of roughness al > 0 (not an interface): the draw of stream
// kGlossStream + d; g = 0 with ended when nd is not above ns; sm: the hit is smooth, and the mirror's two ending rules apply as well.
// NOT inlined, on purpose: a real call keeps the draw's ~200 instructions and its double arithmetic out of the register allocation of
// the path kernels, which are at their VGPR limit.  Inlined, one instantiation (k_pt_filter<1, false, 3, MisArgs, GlossArgs, NormArgs,
// CamArgs>) came out with a stage 1 of the default scan that rejected genuine hits
__device__ __attribute__((noinline)) void gloss_hit(const KArgs& a, uint32_t pixel, uint32_t sample, int depth, float al, f3 dir, f3 ns, f3 n, bool sm, f3& nd, float& g, bool& ended) {
	double u1, u2;
	philox_uniforms(a.seed, pixel, sample, kGlossStream + (uint32_t)depth, &u1, &u2);
	f3 m;
	const bool ok = gloss_bounce(dir, ns, al, u1, u2, m, nd, g);
	if (!ok) g = 0.0f;
	ended = !ok || (sm && (!(dot3(dir, ns) < 0.0f) || dot3(nd, n) < 0.0f));
}
// one step of the unwind with a roughness table: glass_unwind's step, scaled once more by g after a glossy hit (a specular hit whose
// cosine slot ct holds g > 0; a mirror's, an interface's and an ended glossy hit's hold 0)
SP_DEV f3 gloss_unwind(const float4* __restrict__ glass, const float4* __restrict__ spec, int id, f3 e, f3 brdf, f3 rec, float ct) {
	const int i = id & ~(kSpecBit | kTransBit);
	if ((id & kSpecBit) && ct > 0.0f) {
		const float4 q = spec[i];
		return add3(e, scale3(scale3(mul3(mk3(q.x, q.y, q.z), rec), 1.0f / q.w), ct));
	}
	return glass_unwind(glass, spec, id, e, brdf, rec, ct);
}

// ---- textures (include/spath_hip.h "textures").  f32, every operation rounded on its own.
// One axis of the bilinear footprint of coordinate s on n texels, repeat addressing: the two texel indices and the weight of the second
SP_DEV void tex_axis(float s, uint32_t n, int& i0, int& i1, float& fx) {
	float fs = s - __builtin_floorf(s);
	fs = fs < 1.0f ? fs : 0.0f;                        // a small negative s rounds s - floorf(s) up to 1
	const float x = fs * (float)n - 0.5f;
	const float x0 = __builtin_floorf(x);
	fx = x - x0;
	i0 = (int)x0;
	i0 = i0 < 0 ? i0 + (int)n : i0;
	i1 = i0 + 1 == (int)n ? 0 : i0 + 1;
}
// the bilinear sample of the tw x th atlas at (s, t), both finite.  The lerp form returns a texel bit for bit where the four texels of
// the footprint are equal
SP_DEV f3 tex_sample(const float* __restrict__ atlas, uint32_t tw, uint32_t th, float s, float t) {
	int i0, i1, j0, j1;
	float fx, fy;
	tex_axis(s, tw, i0, i1, fx);
	tex_axis(t, th, j0, j1, fy);
	const float* p00 = atlas + ((size_t)j0 * tw + (size_t)i0) * 3;
	const float* p10 = atlas + ((size_t)j0 * tw + (size_t)i1) * 3;
	const float* p01 = atlas + ((size_t)j1 * tw + (size_t)i0) * 3;
	const float* p11 = atlas + ((size_t)j1 * tw + (size_t)i1) * 3;
	float c[3];
#pragma unroll
	for (int k = 0; k < 3; ++k) {
		const float top = p00[k] + (p10[k] - p00[k]) * fx;
		const float bot = p01[k] + (p11[k] - p01[k]) * fx;
		c[k] = top + (bot - top) * fy;
	}
	return mk3(c[0], c[1], c[2]);
}
// the texture's colour c at the hit of ray (o, dir) on the triangle whose vertices are tv[0..8] and whose UV row is uvr[0..5]:
//   bary:    u, v exactly as shade_normal computes them (geom.h:200-212), for the winning triangle
//   interp:  w = (1 - u) - v;  s = (s0 w + s1 u) + s2 v;  t likewise
// Returns whether the hit is textured: the row is not all zero and s, t are finite; otherwise c = 1
SP_DEV bool tex_lookup(const float* __restrict__ tv, const float* __restrict__ uvr, const float* __restrict__ atlas, uint32_t tw, uint32_t th,
                       f3 o, f3 dir, float& s, float& t, f3& c) {
	const f3 v0 = mk3(tv[0], tv[1], tv[2]);
	const f3 e1 = sub3(mk3(tv[3], tv[4], tv[5]), v0), e2 = sub3(mk3(tv[6], tv[7], tv[8]), v0);   // geom.h:200-201
	const f3 h = cross3(dir, e2);                    // :202
	const float a = dot3(e1, h);                     // :203
	const float f = recip_ieee(a);                   // :206
	const f3 sv = sub3(o, v0);                       // :207
	const float u = f * dot3(sv, h);                 // :208
	const f3 q = cross3(sv, e1);                     // :211
	const float v = f * dot3(dir, q);                // :212
	const float w = (1.0f - u) - v;
	s = (uvr[0] * w + uvr[2] * u) + uvr[4] * v;
	t = (uvr[1] * w + uvr[3] * u) + uvr[5] * v;
	const bool zero = uvr[0] == 0.0f && uvr[1] == 0.0f && uvr[2] == 0.0f && uvr[3] == 0.0f && uvr[4] == 0.0f && uvr[5] == 0.0f;
	const bool tex = !zero && fabsf(s) < __builtin_inff() && fabsf(t) < __builtin_inff();
	c = mk3(1.0f, 1.0f, 1.0f);
	if (tex) c = tex_sample(atlas, tw, th, s, t);
	return tex;
}
// the albedo of that hit: rho * c per channel, the material's reflectance rho = mat[0..2] itself on an untextured hit.  Called once per
// hit, after the scan.  NOT inlined, on purpose, as gloss_hit is not: the path kernels are at their VGPR limit
__device__ __attribute__((noinline)) f3 tex_albedo(const float* __restrict__ tv, const float* __restrict__ uvr, const float* __restrict__ mat,
                                                   const float* __restrict__ atlas, uint32_t tw, uint32_t th, f3 o, f3 dir) {
	const f3 rho = mk3(mat[0], mat[1], mat[2]);
	float s, t;
	f3 c;
	if (!tex_lookup(tv, uvr, atlas, tw, th, o, dir, s, t, c)) return rho;
	return mul3(rho, c);
}
// ... for hit triangle bi of a path kernel
SP_DEV f3 tex_hit(const KArgs& a, const TexArgs& x, int bi, f3 o, f3 dir) {
	return tex_albedo(a.tris + (size_t)bi * 12, x.uv + (size_t)bi * 6, a.mats + (size_t)bi * 6, x.atlas, x.tw, x.th, o, dir);
}

// ---- normal mapping (include/spath_hip.h "normal mapping").  f32, every operation rounded on its own.
// The shading normal of the hit of ray (o, dir) on the triangle whose vertices are tv[0..8] and whose UV row is uvr[0..5]; n is the stored
// normal turned against dir, ns what shade_normal left.
//   bary, s, t, texel:  tex_lookup on the map: m = the bilinear sample at the hit's (s, t)
//   frame:   e1 = v1 - v0;  e2 = v2 - v0;  ds1 = s1 - s0;  ds2 = s2 - s0;  dt1 = t1 - t0;  dt2 = t2 - t0
//            det = ds1 dt2 - ds2 dt1;  sg = det < 0 ? -1 : 1;  T = (e1 dt2 - e2 dt1) sg;  B = (e2 ds1 - e1 ds2) sg
//            Tp = T - ns dot3(ns, T);  lt = dot3(Tp, Tp);  Tn = Tp / sqrtf(lt);  C = cross3(ns, Tn);  h = dot3(C, B) < 0 ? -1 : 1;  Bn = C h
//   normal:  p = (Tn m.x + Bn m.y) + ns m.z;  lp = dot3(p, p);  np = p / sqrtf(lp)
// Returns {np, 1} where the hit is perturbed: a textured row, det != 0, lt and lp > 0 and finite, m not (0, 0, z), m.z > 0, np on n's
// side and against dir; {ns, 0} otherwise.  Called once per hit, after shade_normal.  NOT inlined, on purpose, as tex_albedo is not
__device__ __attribute__((noinline)) float4 nmap_normal(const float* __restrict__ tv, const float* __restrict__ uvr, const float* __restrict__ nmap,
                                                        uint32_t nw, uint32_t nh, f3 o, f3 dir, f3 n, f3 ns) {
	float s, t;
	f3 m;
	const float4 keep = make_float4(ns.x, ns.y, ns.z, 0.0f);
	if (!tex_lookup(tv, uvr, nmap, nw, nh, o, dir, s, t, m)) return keep;
	const f3 v0 = mk3(tv[0], tv[1], tv[2]);
	const f3 e1 = sub3(mk3(tv[3], tv[4], tv[5]), v0), e2 = sub3(mk3(tv[6], tv[7], tv[8]), v0);
	const float ds1 = uvr[2] - uvr[0], ds2 = uvr[4] - uvr[0], dt1 = uvr[3] - uvr[1], dt2 = uvr[5] - uvr[1];
	const float det = ds1 * dt2 - ds2 * dt1;
	if (!(det > 0.0f || det < 0.0f)) return keep;
	if ((m.x == 0.0f && m.y == 0.0f) || !(m.z > 0.0f)) return keep;
	const float sg = det < 0.0f ? -1.0f : 1.0f;
	const f3 T = scale3(sub3(scale3(e1, dt2), scale3(e2, dt1)), sg), B = scale3(sub3(scale3(e2, ds1), scale3(e1, ds2)), sg);
	const f3 Tp = sub3(T, scale3(ns, dot3(ns, T)));
	const float lt = dot3(Tp, Tp);
	if (!(lt > 0.0f && lt < __builtin_inff())) return keep;
	const float l = __builtin_sqrtf(lt);
	const f3 Tn = mk3(Tp.x / l, Tp.y / l, Tp.z / l);
	const f3 C = cross3(ns, Tn);
	const f3 Bn = scale3(C, dot3(C, B) < 0.0f ? -1.0f : 1.0f);
	const f3 p = add3(add3(scale3(Tn, m.x), scale3(Bn, m.y)), scale3(ns, m.z));
	const float lp = dot3(p, p);
	if (!(lp > 0.0f && lp < __builtin_inff())) return keep;
	const float q = __builtin_sqrtf(lp);
	const f3 np = mk3(p.x / q, p.y / q, p.z / q);
	if (!(dot3(np, n) > 0.0f) || !(dot3(dir, np) < 0.0f)) return keep;
	return make_float4(np.x, np.y, np.z, 1.0f);
}
// ... for hit triangle bi of a path kernel: ns and sm as shade_normal left them become the hit's
SP_DEV void nmap_hit(const KArgs& a, const NmapArgs& x, int bi, f3 o, f3 dir, f3 n, f3& ns, bool& sm) {
	const float4 r = nmap_normal(a.tris + (size_t)bi * 12, x.uv + (size_t)bi * 6, x.nmap, x.nw, x.nh, o, dir, n, ns);
	ns = mk3(r.x, r.y, r.z);
	sm = sm || r.w != 0.0f;
}

// ---- what the kernels share around the integrator: each is used where the kernel keeps its instructions with it (DESIGN.md
// section 5.9 lists the sites that keep their own lines)

// ray kk of the launch (the caller clamps kk below n_rays)
SP_DEV void load_ray(const KArgs& a, uint32_t kk, f3& o, f3& dir) {
	const float* r = a.rays + (size_t)kk * 6;
	o = mk3(r[0], r[1], r[2]); dir = mk3(r[3], r[4], r[5]);
}

// renderer::render_flat's pixel (cpu_renderer.cpp:89-96): the nearest triangle's reflectance, RGBA{0,0,0,0} for a miss
SP_DEV uint32_t flat_px(const KArgs& a, int bi) {
	uint32_t px = 0;
	if (bi >= 0) {
		const float* m = a.mats + (size_t)bi * 6;
		px = vec3_rgba(mk3(m[0], m[1], m[2]));
	}
	return px;
}

// cpu_renderer.cpp:78: the mean clamped to [0, 1] and quantised to RGBA8
SP_DEV uint32_t clamped_rgba(f3 v) { return vec3_rgba(mk3(clamp01(v.x), clamp01(v.y), clamp01(v.z))); }

} // namespace sp
