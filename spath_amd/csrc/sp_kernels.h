// Kernels of the spath hot path for gfx950 (CDNA4): triangle repack, flat pass, path tracer.
//
// Work decomposition: one lane owns one pixel for the whole integrator -- or, in a
// sample-chunked launch of the filter kernels, for one contiguous range of its samples, with k_resolve adding
// the per-sample results up -- so samples are accumulated in the reference's order (cpu_renderer.cpp:74-76); a wavefront walks 64
// paths in lock-step through the (wave-uniform) depth loop, and the closest-hit scan streams the
// repacked triangle array once per (wave, bounce).
#pragma once

#include "sp_integrator.h"

namespace sp {

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
	a.out_rgba[k] = clamped_rgba(av);
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
		((uint32_t*)out)[i] = clamped_rgba(mk3(q[0], q[1], q[2]));
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

// what 8: dielectric.  dir ns ior entering(0/1) -> Fr tir(0/1) nt.xyz c
__global__ void __launch_bounds__(256) k_selftest_glass(const float* __restrict__ in, uint32_t n, float* __restrict__ out) {
	const uint32_t i = blockIdx.x * 256u + threadIdx.x;
	if (i >= n) return;
	const float* q = in + 8 * (size_t)i;
	float Fr, c;
	bool tir;
	f3 nt;
	dielectric(mk3(q[0], q[1], q[2]), mk3(q[3], q[4], q[5]), q[6], q[7] != 0.0f, Fr, tir, nt, c);
	float* w = out + 6 * (size_t)i;
	w[0] = Fr; w[1] = tir ? 1.0f : 0.0f; w[2] = nt.x; w[3] = nt.y; w[4] = nt.z; w[5] = c;
}

// what 11: gloss_bounce.  dir ns alpha u1 u2 (the f32 values carried in doubles) -> m.xyz nd.xyz g ok
__global__ void __launch_bounds__(256) k_selftest_gloss(const double* __restrict__ in, uint32_t n, float* __restrict__ out) {
	const uint32_t i = blockIdx.x * 256u + threadIdx.x;
	if (i >= n) return;
	const double* q = in + 9 * (size_t)i;
	f3 m, nd;
	float g;
	const bool ok = gloss_bounce(mk3((float)q[0], (float)q[1], (float)q[2]), mk3((float)q[3], (float)q[4], (float)q[5]), (float)q[6], q[7], q[8], m, nd, g);
	float* w = out + 8 * (size_t)i;
	w[0] = m.x; w[1] = m.y; w[2] = m.z; w[3] = nd.x; w[4] = nd.y; w[5] = nd.z; w[6] = g; w[7] = ok ? 1.0f : 0.0f;
}

// what 12: tex_lookup, what tex_albedo samples.  pos dir v0 v1 v2 uv0 uv1 uv2 -> s t c.rgb textured
__global__ void __launch_bounds__(256) k_selftest_tex(const float* __restrict__ in, uint32_t n, const float* __restrict__ atlas, uint32_t tw, uint32_t th, float* __restrict__ out) {
	const uint32_t i = blockIdx.x * 256u + threadIdx.x;
	if (i >= n) return;
	const float* q = in + 21 * (size_t)i;
	float s, t;
	f3 c;
	const bool tx = tex_lookup(q + 6, q + 15, atlas, tw, th, mk3(q[0], q[1], q[2]), mk3(q[3], q[4], q[5]), s, t, c);
	float* w = out + 6 * (size_t)i;
	w[0] = s; w[1] = t; w[2] = c.x; w[3] = c.y; w[4] = c.z; w[5] = tx ? 1.0f : 0.0f;
}

// what 13: nmap_normal after shade_normal.  pos dir v0 v1 v2 n0 n1 n2 uv0 uv1 uv2 -> s t ns.xyz perturbed; the stored normal as in what 7
__global__ void __launch_bounds__(256) k_selftest_nmap(const float* __restrict__ in, uint32_t n, const float* __restrict__ nmap, uint32_t nw, uint32_t nh, float* __restrict__ out) {
	const uint32_t i = blockIdx.x * 256u + threadIdx.x;
	if (i >= n) return;
	const float* q = in + 30 * (size_t)i;
	const f3 o = mk3(q[0], q[1], q[2]), dir = mk3(q[3], q[4], q[5]), v0 = mk3(q[6], q[7], q[8]);
	const f3 c = cross3(sub3(mk3(q[9], q[10], q[11]), v0), sub3(mk3(q[12], q[13], q[14]), v0));
	const float l = __builtin_sqrtf(dot3(c, c));
	f3 nn = mk3(c.x / l, c.y / l, c.z / l);
	if (dot3(nn, dir) > 0.0f) nn = scale3(nn, -1.0f);
	f3 ns, m;
	float s, t;
	(void)shade_normal(q + 6, q + 15, o, dir, nn, ns);
	(void)tex_lookup(q + 6, q + 24, nmap, nw, nh, o, dir, s, t, m);
	const float4 r = nmap_normal(q + 6, q + 24, nmap, nw, nh, o, dir, nn, ns);
	float* w = out + 6 * (size_t)i;
	w[0] = s; w[1] = t; w[2] = r.x; w[3] = r.y; w[4] = r.z; w[5] = r.w;
}

SP_DEV uint64_t shard_pixel(const KArgs& a, uint32_t k) {
	const uint64_t t = (uint64_t)k / a.tile_px;
	return a.pixel_base + t * a.tile_stride_px + ((uint64_t)k - t * a.tile_px);
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
	f3 o, dir;
	load_ray(a, kk, o, dir);
	float bd; int bi;
	closest_hit<VARIANT>(a, o, dir, -1, bd, bi);
	const uint32_t px = flat_px(a, bi);
	if (valid) a.out_rgba[k] = px;
	wave_add_scans(a.scans, valid ? 1u : 0u);
}

// ---- the closest-hit scan alone (cpu_renderer.cpp:36-49), one ray per lane
template <int VARIANT>
__global__ void __launch_bounds__(256) k_hit(const KArgs a, const int* __restrict__ src_idx, int* __restrict__ out_idx, float* __restrict__ out_d) {
	const uint32_t k = blockIdx.x * 256u + threadIdx.x;
	const bool valid = k < a.n_rays;
	const uint32_t kk = valid ? k : a.n_rays - 1;
	f3 o, dir;
	load_ray(a, kk, o, dir);
	float bd; int bi;
	closest_hit<VARIANT>(a, o, dir, src_idx ? src_idx[kk] : -1, bd, bi);
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
	if constexpr (!cam) {                                        // load_ray, written out: the call moves this kernel's instructions (tools/listing_diff.py)
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
	constexpr bool gls = IsGlass<Acc...>::value;                 // transparency (GlassArgs, in SpecArgs' place): kTransBit beside kSpecBit
	static_assert(!gls || VARIANT == 1, "transparency: variant 1 (DESIGN.md section 5.10)");
	constexpr bool env = IsEnv<Acc...>::value;                   // environment lighting (EnvArgs, in GlassArgs' place): a miss carries the map's radiance
	static_assert(!env || mis || !nee, "environment lighting: plain or NEE|MIS (DESIGN.md section 5.11)");
	constexpr bool glo = IsGloss<Acc...>::value;                 // glossy reflection (GlossArgs, in EnvArgs' place): the weight g in the mirror hit's cosine slot
	constexpr bool tex = IsTex<Acc...>::value;                   // textures (TexArgs, in GlossArgs' place): the hit's albedo per depth in A0..A4
	constexpr bool nmp = IsNmap<Acc...>::value;                  // normal mapping (NmapArgs, in TexArgs' place, always with NormArgs): ns from the map
	static_assert(!nmp || smo, "a normal-mapped pack carries NormArgs (DESIGN.md section 5.16)");
	constexpr int hmask = HistMask<Acc...>::value;
	const uint32_t pk = adapt ? local_px(kk, acc_args...) : kk;   // where the pixel's running sums live (valid rays)
	const uint32_t pixel = (uint32_t)shard_pixel(a, pk);
	const bool reuse = !cam && (a.flags & 0x100u) != 0;          // the host rejects reuse with camera samples

	uint32_t my_scans = 0;
	// optional primary-hit reuse: the primary ray is the same for every sample (:74-76)
	float pd = 0.0f; int pi = -1;
	if (reuse) { closest_hit<VARIANT>(a, po, pdir, -1, pd, pi); my_scans += valid ? 1u : 0u; }

	f3 accum = mk3(0.0f, 0.0f, 0.0f);
	double s1 = 0.0, s2 = 0.0;                                   // adaptive: S1, S2 of the pixel (sp_integrator.h AdaptArgs)
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
		f3 Em = L0;                                                  // environment: what the ray that left the scene carries
		f3 A0 = L0, A1 = L0, A2 = L0, A3 = L0, A4 = L0;             // textures: the albedo of hits 0..4
#pragma unroll 1
		for (int depth = 0; depth < (mis ? kMisDepths : nee ? kNeeDepths : 5); ++depth) {   // :33 depth >= 5 -> black (NEE: the 5th hit carries nothing)
			if (!__syncthreads_or(alive ? 1 : 0)) break;   // block-uniform: the LDS scan has barriers
			float bd; int bi;
			if (depth == 0 && reuse) { bd = pd; bi = pi; }
			else { closest_hit<VARIANT>(a, o, dir, src, bd, bi); my_scans += alive ? 1u : 0u; }
			const bool hit = alive && (bi >= 0);                  // :51 miss -> black
			if constexpr (env) if (alive && bi < 0) Em = env_miss<mis>(env_args(acc_args...).env, dir, depth == 0 || pspec);
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
				if constexpr (nmp) nmap_hit(a, nmap_args(acc_args...), bi, o, dir, n, ns, sm);
				[[maybe_unused]] f3 alb;                          // textures: the hit's albedo
				if constexpr (tex) {
					alb = tex_hit(a, tex_args(acc_args...), bi, o, dir);
					if (depth == 0) A0 = alb; else if (depth == 1) A1 = alb; else if (depth == 2) A2 = alb; else if (depth == 3) A3 = alb; else A4 = alb;
				}
				bool sl = false;                                  // specular: this hit takes the mirror lobe
				float pm = 0.0f;
				float gi = 0.0f;                                  // transparency: the triangle's ior; > 0: an interface, a specular hit
				if constexpr (gls) {
					gi = glass_table(acc_args...)[bi].w;
					if (gi > 0.0f) sl = true;
					else { pm = spec_table(acc_args...)[bi].w; sl = spec_lobe(a.seed, pixel, s0 + s, depth, pm); }
				} else if constexpr (spc) { pm = spec_table(acc_args...)[bi].w; sl = spec_lobe(a.seed, pixel, s0 + s, depth, pm); }
				if constexpr (mis) {
					if (depth == 0 || (spc && pspec)) { const float* m = a.mats + (size_t)bi * 6; De = mk3(m[3], m[4], m[5]); }
					else De = mis_emit(a, mis_tipdf(acc_args...), dir, bd, bi);
					if constexpr (tex) { if (depth < kNeeDepths && !sl) sh = nee_light<true, env, true>(a, nee_args(acc_args...), pixel, s0 + s, depth, add3(o, scale3(dir, bd)), ns, bi, wd, tm, Lc, env_map(acc_args...), &alb); }
					else if (depth < kNeeDepths && !sl) sh = nee_light<true, env>(a, nee_args(acc_args...), pixel, s0 + s, depth, add3(o, scale3(dir, bd)), ns, bi, wd, tm, Lc, env_map(acc_args...));
					if constexpr (smo) sh = sh && smooth_light_ok(sm, wd, n);
					if constexpr (spc) if (sh) Lc = scale3(Lc, 1.0f / (1.0f - pm));   // L_d wD (a diffuse hit: p < 1)
				} else if constexpr (nee) sh = nee_light(a, nee_args(acc_args...), pixel, s0 + s, depth, add3(o, scale3(dir, bd)), n, bi, wd, tm, Lc);
				f3 nd;
				float ct = 0.0f;
				bool tr = false;                                  // transparency: the bounce is a transmission
				if (gls && gi > 0.0f) tr = glass_bounce(a, pixel, s0 + s, depth, bi, gi, dir, ns, sm, nd, ended);
				else if (spc && sl) {
					nd = spec_reflect(dir, ns);
					if constexpr (smo) ended = sm && (!(dot3(dir, ns) < 0.0f) || dot3(nd, n) < 0.0f);
					if constexpr (glo) { const float al = rough_table(acc_args...)[bi]; if (al > 0.0f) gloss_hit(a, pixel, s0 + s, depth, al, dir, ns, n, sm, nd, ct, ended); }
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
				if constexpr (gls) if (tr) bi |= kTransBit;
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
		if constexpr (env) rec = Em;
#pragma unroll
		for (int depth = 4; depth >= 0; --depth) {
			const int id = depth == 0 ? idx0 : depth == 1 ? idx1 : depth == 2 ? idx2 : depth == 3 ? idx3 : idx4;
			const float ct = depth == 0 ? c0 : depth == 1 ? c1 : depth == 2 ? c2 : depth == 3 ? c3 : c4;
			if (id >= 0) {
				const float* m = a.mats + (size_t)(spc ? id & hmask : id) * 6;
				f3 brdf = scale3(mk3(m[0], m[1], m[2]), kInvPi);                           // :63
				if constexpr (tex) brdf = scale3(depth == 0 ? A0 : depth == 1 ? A1 : depth == 2 ? A2 : depth == 3 ? A3 : A4, kInvPi);
				f3 e = mk3(m[3], m[4], m[5]);
				if constexpr (mis) e = depth == 0 ? D0 : depth == 1 ? D1 : depth == 2 ? D2 : depth == 3 ? D3 : D4;   // D_d
				else if constexpr (nee) {                                                   // (e_0 or 0) + L_d
					if (depth > 0) e = mk3(0.0f, 0.0f, 0.0f);
					e = add3(e, depth == 0 ? L0 : depth == 1 ? L1 : depth == 2 ? L2 : L3);
				}
				if constexpr (glo) rec = gloss_unwind(glass_table(acc_args...), spec_table(acc_args...), id, e, brdf, rec, ct);
				else if constexpr (gls) rec = glass_unwind(glass_table(acc_args...), spec_table(acc_args...), id, e, brdf, rec, ct);
				else if constexpr (spc) rec = spec_unwind(spec_table(acc_args...)[id & ~kSpecBit], (id & kSpecBit) != 0, e, brdf, rec, ct);
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
		a.out_rgba[k] = clamped_rgba(accum);                     // :78
		if (a.out_accum) {
			a.out_accum[(size_t)k * 3 + 0] = accum.x;
			a.out_accum[(size_t)k * 3 + 1] = accum.y;
			a.out_accum[(size_t)k * 3 + 2] = accum.z;
		}
	}
	wave_add_scans(a.scans, my_scans);
}

} // namespace sp
