// Kernels of the spath hot path for gfx950 (CDNA4): triangle repack, flat pass, path tracer.
//
// Work decomposition: one lane owns one pixel for the whole integrator -- or, in a
// sample-chunked launch of the filter kernels, for one contiguous range of its samples, with k_resolve adding
// the per-sample results up -- so samples are accumulated in the reference's order (cpu_renderer.cpp:74-76); a wavefront walks 64
// paths in lock-step through the (wave-uniform) depth loop, and the closest-hit scan streams the
// repacked triangle array once per (wave, bounce).
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
template <typename... Acc> struct IsSpec { static constexpr bool value = PackHas<SpecArgs, Acc...>::value; };
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

// second pass of a sample-chunked launch: cpu_renderer.cpp:72-78 for one pixel -- zero, += sample in sample order,
// * float(1.0/n_samples), clamp, quantise
template <typename... Acc>
__global__ void __launch_bounds__(256) k_resolve(const KArgs a, const Acc... acc_args) {
	const uint32_t k = blockIdx.x * 256u + threadIdx.x;
	if (k >= a.n_rays) return;
	constexpr bool adapt = IsAdapt<Acc...>::value;
	const uint32_t pk = local_px(k, acc_args...);             // where the pixel's running sum lives
	float ax = 0.0f, ay = 0.0f, az = 0.0f;
	double s1 = 0.0, s2 = 0.0;
	if constexpr (HasAccum<Acc...>::value) {
		const AccumArgs& q = accum_args(acc_args...);
		if (q.sample_base) { ax = q.sum[(size_t)pk * 3 + 0]; ay = q.sum[(size_t)pk * 3 + 1]; az = q.sum[(size_t)pk * 3 + 2]; }
		if constexpr (adapt) if (q.sample_base) { s1 = adapt_args(acc_args...).s12[(size_t)pk * 2]; s2 = adapt_args(acc_args...).s12[(size_t)pk * 2 + 1]; }
	}
	for (uint32_t s = 0; s < a.n_samples; ++s) {
		const float* p = a.samp + (size_t)s * 3 * a.samp_stride + k;
		const float rx = p[0], ry = p[a.samp_stride], rz = p[(size_t)2 * a.samp_stride];
		ax = ax + rx;
		ay = ay + ry;
		az = az + rz;
		if constexpr (adapt) { const double y = lum_proxy(rx, ry, rz); s1 = s1 + y; s2 = s2 + y * y; }
	}
	if constexpr (HasAccum<Acc...>::value) {
		const AccumArgs& q = accum_args(acc_args...);
		q.sum[(size_t)pk * 3 + 0] = ax; q.sum[(size_t)pk * 3 + 1] = ay; q.sum[(size_t)pk * 3 + 2] = az;
	}
	if constexpr (adapt) {
		adapt_args(acc_args...).s12[(size_t)pk * 2] = s1; adapt_args(acc_args...).s12[(size_t)pk * 2 + 1] = s2;
		return;                                                  // the frame is resolved from sums and counts (k_adapt_resolve)
	}
	const f3 av = scale3(mk3(ax, ay, az), a.inv_n);
	a.out_rgba[k] = vec3_rgba(mk3(clamp01(av.x), clamp01(av.y), clamp01(av.z)));
	if (a.out_accum) {
		a.out_accum[(size_t)k * 3 + 0] = av.x;
		a.out_accum[(size_t)k * 3 + 1] = av.y;
		a.out_accum[(size_t)k * 3 + 2] = av.z;
	}
}

// ---- repack: AoS geom::triangle -> scan records.  e1/e2 are the single float subtractions of
// geom.h:200-201, hoisted out of the per-ray test (same bits).  Also the scene bound Rv (bounds[0], zeroed by the host) that the
// margins of the two-stage scans are built from.
__global__ void __launch_bounds__(256) k_repack(const float* __restrict__ tris, float4* __restrict__ scan, unsigned int* __restrict__ bounds, uint32_t n, uint32_t n_padded) {
	const uint32_t i = blockIdx.x * 256u + threadIdx.x;
	if (i >= n_padded) return;
	if (i >= n) {   // padding record: e1 = e2 = 0 -> a = 0 -> rejected at geom.h:204, can never be hit
		const float4 z = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
		scan[(size_t)i * 3 + 0] = z; scan[(size_t)i * 3 + 1] = z; scan[(size_t)i * 3 + 2] = z;
		return;
	}
	const float* t = tris + (size_t)i * 12;
	const float v0x = t[0], v0y = t[1], v0z = t[2];
	const float e1x = t[3] - v0x, e1y = t[4] - v0y, e1z = t[5] - v0z;
	const float e2x = t[6] - v0x, e2y = t[7] - v0y, e2z = t[8] - v0z;
	scan[(size_t)i * 3 + 0] = make_float4(v0x, v0y, v0z, e1x);
	scan[(size_t)i * 3 + 1] = make_float4(e1y, e1z, e2x, e2y);
	scan[(size_t)i * 3 + 2] = make_float4(e2z, 0.0f, 0.0f, 0.0f);
	// scene bound Rv >= every vertex norm, as 1-norms (>= 2-norm); non-negative floats order like their bit patterns;
	// a NaN or inf coordinate yields a bit pattern >= inf, which turns the filter off in the kernels
	float r = 0.0f;
#pragma unroll
	for (int k = 0; k < 3; ++k) {
		const float s = fabsf(t[3 * k]) + fabsf(t[3 * k + 1]) + fabsf(t[3 * k + 2]);
		r = (s > r || s != s) ? s : r;
	}
	atomicMax(bounds, __float_as_uint(r) & 0x7fffffffu);
}

SP_DEV f3 cam_rel_move(const ViewArgs& v, f3 in) {                               // view.h:83-85 = rY(rX(in))
	const f3 a = mk3(in.x, in.y * v.cos_x + in.z * -v.sin_x, in.y * v.sin_x + in.z * v.cos_x);   // :62-68
	return mk3(a.x * v.cos_y + a.z * v.sin_y, a.y, a.x * -v.sin_y + a.z * v.cos_y);              // :54-60
}

__global__ void __launch_bounds__(256) k_viewport(const ViewArgs v, float* __restrict__ rays) {
	const uint32_t k = blockIdx.x * 256u + threadIdx.x;
	if (k >= v.n_local) return;
	const uint64_t tile = (uint64_t)k / v.tile_px;
	const uint64_t idx = v.pixel_base + tile * v.tile_stride_px + ((uint64_t)k - tile * v.tile_px);
	const int i = (int)(idx % v.res_x), j = (int)(idx / v.res_x);                 // :112 index = i + j*res_x
	const f3 cur = mk3(v.x_max - v.x_step * (float)i - v.h_x_step, v.y_max - v.y_step * (float)j - v.h_y_step, 0.0f);   // :111
	const f3 t = add3(cur, mk3(0.0f, 0.0f, v.focal));                             // :114
	const float l = __builtin_sqrtf(t.x * t.x + t.y * t.y + t.z * t.z);           // geom.h:130-136 (IEEE sqrt)
	const f3 dir = cam_rel_move(v, mk3(t.x / l, t.y / l, t.z / l));               // :138-141 then view.h:127
	const f3 pos = add3(cam_rel_move(v, cur), mk3(v.px, v.py, v.pz));             // view.h:126,131
	float* o = rays + (size_t)k * 6;
	o[0] = pos.x; o[1] = pos.y; o[2] = pos.z; o[3] = dir.x; o[4] = dir.y; o[5] = dir.z;
}

// ---- the primary ray of (global pixel p, global sample) with SPHIP_FLAG_CAMERA_SAMPLES (include/spath_hip.h):
// k_viewport's pinhole ray at a box-filtered position in the pixel and, with a lens, from a point of the lens disk (on the image
// plane) through the point in focus at local z = focus_dist.  f32 throughout except where the reference's own draws are double.
SP_DEV void camera_ray(const CamArgs& c, uint64_t seed, uint32_t p, uint32_t sample, f3& pos, f3& dir) {
	const ViewArgs& v = c.v;
	const uint32_t i = p % v.res_x, j = p / v.res_x;
	double r1, r2;
	philox_uniforms(seed, p, sample, 24u, &r1, &r2);
	const f3 cur = mk3((v.x_max - v.x_step * (float)i) - v.x_step * (float)r1, (v.y_max - v.y_step * (float)j) - v.y_step * (float)r2, 0.0f);
	const f3 t = add3(cur, mk3(0.0f, 0.0f, v.focal));
	f3 o = cur, g = t;
	if (c.aperture > 0.0f) {
		double r3, r4;
		philox_uniforms(seed, p, sample, 25u, &r3, &r4);
		const float rho = c.aperture * (float)__builtin_sqrt(r3);
		const float phi = (float)((r4 * kPi) * 2.0);                 // as geom.h:167
		float sn, cs;
		sincos_glibc(phi, &sn, &cs);
		o = mk3(cur.x + rho * cs, cur.y + rho * sn, 0.0f);
		const float kf = c.focus_dist / v.focal;
		g = sub3(add3(cur, scale3(t, kf)), o);                          // F - o, F = cur + t * k
	}
	const float l = __builtin_sqrtf(dot3(g, g));
	dir = cam_rel_move(v, mk3(g.x / l, g.y / l, g.z / l));
	pos = add3(cam_rel_move(v, o), mk3(v.px, v.py, v.pz));
}

// sphip_camera_rays_device: the rays of one sample for the whole image, ray k = global pixel k
__global__ void __launch_bounds__(256) k_camera_rays(const CamArgs c, uint64_t seed, uint32_t sample, float* __restrict__ rays) {
	const uint32_t k = blockIdx.x * 256u + threadIdx.x;
	if (k >= c.v.n_local) return;
	f3 pos, dir;
	camera_ray(c, seed, k, sample, pos, dir);
	float* o = rays + (size_t)k * 6;
	o[0] = pos.x; o[1] = pos.y; o[2] = pos.z; o[3] = dir.x; o[4] = dir.y; o[5] = dir.z;
}

// ---- reassembly of a frame rendered as interleaved row tiles on G devices (one padded buffer of `pad` pixels per device,
// gathered to one device): out[p] = the p-th pixel of the image.  C = dwords per pixel (1: RGBA8, 3: float accumulators)
template <int C>
__global__ void __launch_bounds__(256) k_assemble(const uint32_t* __restrict__ gathered, uint32_t* __restrict__ out, uint32_t npix,
                                                 uint32_t tile_px, uint32_t n_dev, uint32_t pad) {
	const uint32_t p = blockIdx.x * 256u + threadIdx.x;
	if (p >= npix) return;
	const uint32_t tile = p / tile_px, r = tile % n_dev, k = (tile / n_dev) * tile_px + (p - tile * tile_px);
#pragma unroll
	for (int c = 0; c < C; ++c) out[(size_t)p * C + c] = gathered[((size_t)r * pad + k) * C + c];
}

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

// ---- test-only: the device functions of the path on caller-supplied inputs (include/spath_hip.h: sphip_selftest_device)
__global__ void __launch_bounds__(256) k_selftest(int what, const void* __restrict__ in, uint32_t n, void* __restrict__ out) {
	const uint32_t i = blockIdx.x * 256u + threadIdx.x;
	if (i >= n) return;
	if (what == 0) {
		float sn, cs;
		sincos_glibc(((const float*)in)[i], &sn, &cs);
		((float*)out)[2 * i] = sn; ((float*)out)[2 * i + 1] = cs;
	} else if (what == 1) {
		((float*)out)[i] = recip_ieee(((const float*)in)[i]);
	} else if (what == 2) {
		const uint32_t* q = (const uint32_t*)in + 5 * (size_t)i;
		double r1, r2;
		philox_uniforms((uint64_t)q[0] | ((uint64_t)q[1] << 32), q[2], q[3], q[4], &r1, &r2);
		((double*)out)[2 * i] = r1; ((double*)out)[2 * i + 1] = r2;
	} else if (what == 3) {
		const double* q = (const double*)in + 5 * (size_t)i;
		const f3 v = rand_unit_vec(mk3((float)q[0], (float)q[1], (float)q[2]), q[3], q[4]);
		float* o = (float*)out + 3 * (size_t)i;
		o[0] = v.x; o[1] = v.y; o[2] = v.z;
	} else if (what == 4) {
		const float* q = (const float*)in + 15 * (size_t)i;
		const f3 v0 = mk3(q[6], q[7], q[8]);
		// e1, e2 as k_repack forms them: one float subtraction each (geom.h:200-201)
		((float*)out)[i] = ray_tri_strict(mk3(q[0], q[1], q[2]), mk3(q[3], q[4], q[5]), v0, sub3(mk3(q[9], q[10], q[11]), v0), sub3(mk3(q[12], q[13], q[14]), v0));
	} else if (what == 5) {
		const float* q = (const float*)in + 3 * (size_t)i;
		((uint32_t*)out)[i] = vec3_rgba(mk3(clamp01(q[0]), clamp01(q[1]), clamp01(q[2])));
	}
}

// what 7: shade_normal.  pos dir v0 v1 v2 n0 n1 n2 -> u v ns.xyz sm; the stored normal is geom::flat_normal of the vertices (geom.h:192-195)
__global__ void __launch_bounds__(256) k_selftest_shade(const float* __restrict__ in, uint32_t n, float* __restrict__ out) {
	const uint32_t i = blockIdx.x * 256u + threadIdx.x;
	if (i >= n) return;
	const float* q = in + 24 * (size_t)i;
	const f3 o = mk3(q[0], q[1], q[2]), dir = mk3(q[3], q[4], q[5]), v0 = mk3(q[6], q[7], q[8]);
	const f3 c = cross3(sub3(mk3(q[9], q[10], q[11]), v0), sub3(mk3(q[12], q[13], q[14]), v0));
	const float l = __builtin_sqrtf(dot3(c, c));
	f3 nn = mk3(c.x / l, c.y / l, c.z / l);
	if (dot3(nn, dir) > 0.0f) nn = scale3(nn, -1.0f);
	f3 ns;
	float uv[2];
	const bool sm = shade_normal(q + 6, q + 15, o, dir, nn, ns, uv);
	float* w = out + 6 * (size_t)i;
	w[0] = uv[0]; w[1] = uv[1]; w[2] = ns.x; w[3] = ns.y; w[4] = ns.z; w[5] = sm ? 1.0f : 0.0f;
}

SP_DEV uint64_t shard_pixel(const KArgs& a, uint32_t k) {
	const uint64_t t = (uint64_t)k / a.tile_px;
	return a.pixel_base + t * a.tile_stride_px + ((uint64_t)k - t * a.tile_px);
}

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

// ---- next-event estimation: one light sample at the hit x of a path (include/spath_hip.h).
// n: the hit triangle's normal as the path uses it (turned against the incoming ray); src: the hit triangle.  Returns whether a
// shadow ray (x, wd) with the bound tmax is to be traced, and then L = the direct light it carries when nothing occludes it.
// MIS: L carries the balance heuristic's weight u / (1 + u), and sxz = 0 is no early-out (L is finite).
template <bool MIS = false>
SP_DEV bool nee_light(const KArgs& a, const NeeArgs& ne, uint32_t pixel, uint32_t sample, int depth, f3 x, f3 n, int src,
                      f3& wd, float& tmax, f3& L) {
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
	L = mul3(scale3(mk3(ms[0], ms[1], ms[2]), kInvPi), scale3(mk3(me[3], me[4], me[5]), g));
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

// ---- closest-hit scan, variant "rpl_sload": ray per lane, triangle index wave-uniform so the
// records arrive through the scalar data path (s_load_dwordx4) and every VALU op reads them as
// SGPR operands.  Semantics of cpu_renderer.cpp:36-49: ascending index, strict '<', skip idx_source.
// tmax < kMaxDist: the bounded (shadow) form of the same scan -- only hits with d < tmax count (sp_cylm_scan.h, scan_cylm)
SP_DEV void scan_rpl_sload(const float4* __restrict__ scan, uint32_t n_tris, f3 o, f3 dir, int src,
                           float& best_d, int& best_i, float tmax = kMaxDist) {
	float bd = tmax;
	int bi = -1;
	for (uint32_t j = 0; j < n_tris; ++j) {
		const float4 q0 = scan[3 * j + 0], q1 = scan[3 * j + 1], q2 = scan[3 * j + 2];
		const f3 v0 = mk3(q0.x, q0.y, q0.z), e1 = mk3(q0.w, q1.x, q1.y), e2 = mk3(q1.z, q1.w, q2.x);
		const float d = ray_tri_strict(o, dir, v0, e1, e2);
		const bool take = (d > 0.0f) && (d < bd) && ((int)j != src);
		bd = take ? d : bd;
		bi = take ? (int)j : bi;
	}
	best_d = bd;
	best_i = bi;
}

// ---- closest-hit scan, variant "rpl_lds": ray per lane; the workgroup streams the scan records
// HBM/L2 -> registers -> LDS in coalesced 16-byte pieces (double-buffered tiles of kTile triangles),
// and every lane reads the current triangle from LDS at a wave-uniform address (hardware broadcast),
// so all VALU operands are VGPRs.  One triangle fetched from L2/HBM is shared by the 256 rays of the
// workgroup.  Must be called by every thread of the block.
constexpr int kTile = 256;                      // triangles per LDS tile (12 KB), two tiles in flight
constexpr int kTileQ = kTile * 3;               // float4 per tile
static_assert(kTileQ % 256 == 0, "tile must split evenly over the 256 threads");

SP_DEV void scan_rpl_lds(const float4* __restrict__ scan, uint32_t n_tris, f3 o, f3 dir, int src,
                         float& best_d, int& best_i, float tmax = kMaxDist) {
	__shared__ float4 sm[2 * kTileQ];
	static_assert(kTileQ == 3 * 256, "three float4 per thread per tile");
	const uint32_t tid = threadIdx.x;
	const uint32_t ntiles = (n_tris + kTile - 1) / kTile;   // the scan buffer is zero-padded to whole tiles
	float4 p0 = scan[tid], p1 = scan[256 + tid], p2 = scan[512 + tid];
	__syncthreads();                            // readers of the previous scan are done with sm
	sm[tid] = p0; sm[256 + tid] = p1; sm[512 + tid] = p2;
	__syncthreads();
	float bd = tmax;
	int bi = -1;
	for (uint32_t t = 0; t < ntiles; ++t) {
		const float4* cur = sm + (t & 1u) * kTileQ;
		const bool more = (t + 1 < ntiles);
		const float4* nsrc = scan + (size_t)(more ? t + 1 : t) * kTileQ;   // last tile: harmless re-read
		p0 = nsrc[tid]; p1 = nsrc[256 + tid]; p2 = nsrc[512 + tid];
		const uint32_t left = n_tris - t * kTile;
		const uint32_t cnt = ((left < (uint32_t)kTile ? left : (uint32_t)kTile) + 3u) & ~3u;   // zero records never hit
		const int base = (int)(t * kTile);
#pragma unroll 4
		for (uint32_t j = 0; j < cnt; ++j) {
			const float4 q0 = cur[3 * j + 0], q1 = cur[3 * j + 1], q2 = cur[3 * j + 2];
			const f3 v0 = mk3(q0.x, q0.y, q0.z), e1 = mk3(q0.w, q1.x, q1.y), e2 = mk3(q1.z, q1.w, q2.x);
			const float d = ray_tri_strict(o, dir, v0, e1, e2);
			const int idx = base + (int)j;
			const bool take = (d > 0.0f) && (d < bd) && (idx != src);
			bd = take ? d : bd;
			bi = take ? idx : bi;
		}
		float4* nxt = sm + ((t + 1) & 1u) * kTileQ;   // not read before the barrier below + the next one
		nxt[tid] = p0; nxt[256 + tid] = p1; nxt[512 + tid] = p2;
		__syncthreads();
	}
	best_d = bd;
	best_i = bi;
}

// VARIANT 1 = rpl_sload, 2 = rpl_lds.  Every variant must be called block-uniformly.
template <int VARIANT>
SP_DEV void closest_hit(const KArgs& a, f3 o, f3 dir, int src, float& best_d, int& best_i, float tmax = kMaxDist) {
	if (VARIANT == 2) scan_rpl_lds(a.scan, a.n_tris, o, dir, src, best_d, best_i, tmax);
	else scan_rpl_sload(a.scan, a.n_tris, o, dir, src, best_d, best_i, tmax);
}

SP_DEV void wave_add_scans(unsigned long long* ctr, uint32_t mine) {
	// one atomic per wavefront
	uint32_t v = mine;
#pragma unroll
	for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
	if ((threadIdx.x & 63u) == 0 && v) atomicAdd(ctr, (unsigned long long)v);
}

// ---- renderer::render_flat (cpu_renderer.cpp:81-101): nearest triangle's reflectance, no skip
template <int VARIANT>
__global__ void __launch_bounds__(256) k_flat(const KArgs a) {
	const uint32_t k = blockIdx.x * 256u + threadIdx.x;
	const bool valid = k < a.n_rays;
	const uint32_t kk = valid ? k : a.n_rays - 1;
	const float* r = a.rays + (size_t)kk * 6;
	const f3 o = mk3(r[0], r[1], r[2]), dir = mk3(r[3], r[4], r[5]);
	float bd; int bi;
	closest_hit<VARIANT>(a, o, dir, -1, bd, bi);
	uint32_t px = 0;                                             // :89 RGBA{0,0,0,0}
	if (bi >= 0) {
		const float* m = a.mats + (size_t)bi * 6;
		px = vec3_rgba(mk3(m[0], m[1], m[2]));                   // :96
	}
	if (valid) a.out_rgba[k] = px;
	wave_add_scans(a.scans, valid ? 1u : 0u);
}

// ---- the closest-hit scan alone (cpu_renderer.cpp:36-49), one ray per lane
template <int VARIANT>
__global__ void __launch_bounds__(256) k_hit(const KArgs a, const int* __restrict__ src_idx, int* __restrict__ out_idx, float* __restrict__ out_d) {
	const uint32_t k = blockIdx.x * 256u + threadIdx.x;
	const bool valid = k < a.n_rays;
	const uint32_t kk = valid ? k : a.n_rays - 1;
	const float* r = a.rays + (size_t)kk * 6;
	float bd; int bi;
	closest_hit<VARIANT>(a, mk3(r[0], r[1], r[2]), mk3(r[3], r[4], r[5]), src_idx ? src_idx[kk] : -1, bd, bi);
	if (valid) { out_idx[k] = bi; out_d[k] = bd; }
	wave_add_scans(a.scans, valid ? 1u : 0u);
}

// ---- renderer::render (cpu_renderer.cpp:29-79): n_samples x (<=5 surface hits).
// The recursion of render_step is run forward (store idx and cos(theta) per depth) and unwound
// backward in the reference's own evaluation order  E + (((BRDF*rec)*cos)*(1/p))  (:67) -- the
// shape the reference itself uses in its GLSL backend (render.comp:160-215).
template <int VARIANT, typename... Acc>
__global__ void __launch_bounds__(256) k_pt(const KArgs a, const Acc... acc_args) {
	const uint32_t k = blockIdx.x * 256u + threadIdx.x;
	const bool valid = k < a.n_rays;
	const uint32_t kk = valid ? k : a.n_rays - 1;
	constexpr bool cam = IsCam<Acc...>::value;                   // per-sample camera rays (CamArgs): KArgs::rays is not read
	f3 po = mk3(0.0f, 0.0f, 0.0f), pdir = po;
	if constexpr (!cam) {
		const float* r = a.rays + (size_t)kk * 6;
		po = mk3(r[0], r[1], r[2]); pdir = mk3(r[3], r[4], r[5]);
	}
	constexpr bool adapt = IsAdapt<Acc...>::value;
	constexpr bool nee = IsNee<Acc...>::value;
	constexpr bool mis = IsMis<Acc...>::value;                   // MIS: nee too; the folded terms D_0..D_4
	constexpr bool spc = IsSpec<Acc...>::value;                  // specular reflection (SpecArgs): a mirror lobe per hit, marked by kSpecBit in idx0..4
	static_assert(!spc || mis || !nee, "specular reflection: plain or NEE|MIS (DESIGN.md section 5.7)");
	constexpr bool smo = IsNorm<Acc...>::value;                  // smooth shading (NormArgs): ns of shade_normal shades, n guards
	static_assert(!smo || ((mis || !nee) && VARIANT == 1), "smooth shading: plain or NEE|MIS, variant 1 (DESIGN.md section 5.8)");
	const uint32_t pk = adapt ? local_px(kk, acc_args...) : kk;   // where the pixel's running sums live (valid rays)
	const uint32_t pixel = (uint32_t)shard_pixel(a, pk);
	const bool reuse = !cam && (a.flags & 0x100u) != 0;          // the host rejects reuse with camera samples

	uint32_t my_scans = 0;
	// optional primary-hit reuse: the primary ray is the same for every sample (:74-76)
	float pd = 0.0f; int pi = -1;
	if (reuse) { closest_hit<VARIANT>(a, po, pdir, -1, pd, pi); my_scans += valid ? 1u : 0u; }

	f3 accum = mk3(0.0f, 0.0f, 0.0f);
	double s1 = 0.0, s2 = 0.0;                                   // adaptive: S1, S2 of the pixel (sp_kernels.h AdaptArgs)
	uint32_t s0 = 0;                                             // global index of the launch's first sample
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
		int src = -1;
		int idx0 = -1, idx1 = -1, idx2 = -1, idx3 = -1, idx4 = -1;
		float c0 = 0.0f, c1 = 0.0f, c2 = 0.0f, c3 = 0.0f, c4 = 0.0f;
		bool alive = valid;
		bool pspec = false;                                          // specular: the previous hit took the mirror lobe
		f3 L0 = mk3(0.0f, 0.0f, 0.0f), L1 = L0, L2 = L0, L3 = L0;   // NEE: direct light sampled at hits 0..3
		f3 D0 = L0, D1 = L0, D2 = L0, D3 = L0, D4 = L0;             // MIS: D_d = e_d w_b + L_d
#pragma unroll 1
		for (int depth = 0; depth < (mis ? kMisDepths : nee ? kNeeDepths : 5); ++depth) {   // :33 depth >= 5 -> black (NEE: the 5th hit carries nothing)
			if (!__syncthreads_or(alive ? 1 : 0)) break;   // block-uniform: the LDS scan has barriers
			float bd; int bi;
			if (depth == 0 && reuse) { bd = pd; bi = pi; }
			else { closest_hit<VARIANT>(a, o, dir, src, bd, bi); my_scans += alive ? 1u : 0u; }
			const bool hit = alive && (bi >= 0);                  // :51 miss -> black
			bool sh = false;                                      // NEE: this lane traces a shadow ray
			f3 wd = dir, Lc = mk3(0.0f, 0.0f, 0.0f);
			float tm = kMaxDist;
			f3 De = Lc;                                           // MIS: e_d w_b
			bool ended = false;                                   // smooth shading: the bounce left the surface's upper side, the path ends here
			if (hit) {
				const float* tn = a.tris + (size_t)bi * 12 + 9;
				f3 n = mk3(tn[0], tn[1], tn[2]);                  // :55
				if (dot3(n, dir) > 0.0f) n = scale3(n, -1.0f);    // :56-57
				f3 ns = n;                                        // the shading normal
				bool sm = false;
				if constexpr (smo) sm = shade_normal(a.tris + (size_t)bi * 12, norm_table(acc_args...) + (size_t)bi * 9, o, dir, n, ns);
				bool sl = false;                                  // specular: this hit takes the mirror lobe
				float pm = 0.0f;
				if constexpr (spc) { pm = spec_table(acc_args...)[bi].w; sl = spec_lobe(a.seed, pixel, s0 + s, depth, pm); }
				if constexpr (mis) {
					if (depth == 0 || (spc && pspec)) { const float* m = a.mats + (size_t)bi * 6; De = mk3(m[3], m[4], m[5]); }
					else De = mis_emit(a, mis_tipdf(acc_args...), dir, bd, bi);
					if (depth < kNeeDepths && !sl) sh = nee_light<true>(a, nee_args(acc_args...), pixel, s0 + s, depth, add3(o, scale3(dir, bd)), ns, bi, wd, tm, Lc);
					if constexpr (smo) sh = sh && smooth_light_ok(sm, wd, n);
					if constexpr (spc) if (sh) Lc = scale3(Lc, 1.0f / (1.0f - pm));   // L_d wD (a diffuse hit: p < 1)
				} else if constexpr (nee) sh = nee_light(a, nee_args(acc_args...), pixel, s0 + s, depth, add3(o, scale3(dir, bd)), n, bi, wd, tm, Lc);
				f3 nd;
				float ct = 0.0f;
				if (spc && sl) {
					nd = spec_reflect(dir, ns);
					if constexpr (smo) ended = sm && (!(dot3(dir, ns) < 0.0f) || dot3(nd, n) < 0.0f);
				} else {
					double r1, r2;
					philox_uniforms(a.seed, pixel, s0 + s, (uint32_t)depth, &r1, &r2);
					nd = rand_unit_vec(ns, r1, r2);               // :58
					ct = dot3(nd, ns);                            // :62
					if constexpr (smo) ended = sm && dot3(nd, n) < 0.0f;
				}
				o = add3(o, scale3(dir, bd));                     // geom.h:218 point = pos + dir*d
				dir = nd;
				src = bi;
				if constexpr (spc) { pspec = sl; if (sl) bi |= kSpecBit; }
				if (depth == 0) { idx0 = bi; c0 = ct; }
				else if (depth == 1) { idx1 = bi; c1 = ct; }
				else if (depth == 2) { idx2 = bi; c2 = ct; }
				else if (depth == 3) { idx3 = bi; c3 = ct; }
				else { idx4 = bi; c4 = ct; }
			}
			alive = hit && !ended;
			if constexpr (nee) {
				// the shadow rays of the block: (x, wd), skipping the hit triangle, bounded by tmax; any hit occludes
				if (__syncthreads_or(sh ? 1 : 0)) {
					float sd; int si;
					closest_hit<VARIANT>(a, o, wd, src, sd, si, tm);
					my_scans += sh ? 1u : 0u;
					sh = sh && si < 0;
				}
				const f3 Ld = sh ? Lc : mk3(0.0f, 0.0f, 0.0f);
				if constexpr (mis) {
					const f3 Dd = depth < kNeeDepths ? add3(De, Ld) : De;
					if (depth == 0) D0 = Dd; else if (depth == 1) D1 = Dd; else if (depth == 2) D2 = Dd; else if (depth == 3) D3 = Dd; else D4 = Dd;
				} else {
					if (depth == 0) L0 = Ld; else if (depth == 1) L1 = Ld; else if (depth == 2) L2 = Ld; else L3 = Ld;
				}
			}
		}
		// unwind: rec(depth) = E + (((BRDF * rec(depth+1)) * cos) * (1/p)), rec beyond the last hit = 0
		f3 rec = mk3(0.0f, 0.0f, 0.0f);
#pragma unroll
		for (int depth = 4; depth >= 0; --depth) {
			const int id = depth == 0 ? idx0 : depth == 1 ? idx1 : depth == 2 ? idx2 : depth == 3 ? idx3 : idx4;
			const float ct = depth == 0 ? c0 : depth == 1 ? c1 : depth == 2 ? c2 : depth == 3 ? c3 : c4;
			if (id >= 0) {
				const float* m = a.mats + (size_t)(spc ? id & ~kSpecBit : id) * 6;
				const f3 brdf = scale3(mk3(m[0], m[1], m[2]), kInvPi);                     // :63
				f3 e = mk3(m[3], m[4], m[5]);
				if constexpr (mis) e = depth == 0 ? D0 : depth == 1 ? D1 : depth == 2 ? D2 : depth == 3 ? D3 : D4;   // D_d
				else if constexpr (nee) {                                                   // (e_0 or 0) + L_d
					if (depth > 0) e = mk3(0.0f, 0.0f, 0.0f);
					e = add3(e, depth == 0 ? L0 : depth == 1 ? L1 : depth == 2 ? L2 : L3);
				}
				if constexpr (spc) rec = spec_unwind(spec_table(acc_args...)[id & ~kSpecBit], (id & kSpecBit) != 0, e, brdf, rec, ct);
				else rec = add3(e, scale3(scale3(mul3(brdf, rec), ct), kInvP));            // :67
			}
		}
		accum = add3(accum, rec);                                // :75
		if constexpr (adapt) { const double y = lum_proxy(rec.x, rec.y, rec.z); s1 = s1 + y; s2 = s2 + y * y; }
	}
	if constexpr (adapt) {                                       // the frame is resolved from sums and counts (k_adapt_resolve)
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
	accum = scale3(accum, a.inv_n);                              // :77
	if (valid) {
		a.out_rgba[k] = vec3_rgba(mk3(clamp01(accum.x), clamp01(accum.y), clamp01(accum.z)));  // :78
		if (a.out_accum) {
			a.out_accum[(size_t)k * 3 + 0] = accum.x;
			a.out_accum[(size_t)k * 3 + 1] = accum.y;
			a.out_accum[(size_t)k * 3 + 2] = accum.z;
		}
	}
	wave_add_scans(a.scans, my_scans);
}

} // namespace sp
