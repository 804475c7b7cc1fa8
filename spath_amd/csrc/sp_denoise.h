// G-buffer and edge-aware a-trous denoiser (include/spath_hip.h: sphip_gbuffer_device, sphip_denoise_device,
// sphip_accum_denoise).  A post-process: nothing here is reached by the scan or path kernels.
//
// Every operation below is an f32 + - * / (IEEE division), a comparison or a select, in the order the header states, so that a
// numpy model replays the output bit for bit (the build has -ffp-contract=off: nothing is fused).  "max(0, x)" is written
// x > 0 ? x : 0.
//
// Layouts: G-buffer entry = two float4 {nx, ny, nz, dist}, {ar, ag, ab, mat as i32 bits} (32 B, AoS); the filter ping-pongs
// float4 {r, g, b, var} per pixel.
#pragma once

#include "sp_kernels.h"

namespace sp {

// one G-buffer entry per ray from the closest hit (idx, dist) of sphip_closest_hit_device; cls[t] = material class of triangle t.
// With a trailing NormArgs (smooth shading, sp_integrator.h: k_gbuffer_smooth) the normal is the path kernels' shading normal of the primary ray.
template <typename... Norm>
SP_DEV void gbuffer_entry(const float* __restrict__ rays, const int* __restrict__ idx, const float* __restrict__ dist,
                          const float* __restrict__ tris, const float* __restrict__ mats, const int* __restrict__ cls,
                          uint32_t n, float4* __restrict__ out, const Norm... norm) {
	const uint32_t p = blockIdx.x * 256u + threadIdx.x;
	if (p >= n) return;
	const int i = idx[p];
	float4 g0 = make_float4(0.0f, 0.0f, 0.0f, 1e12f), g1 = make_float4(0.0f, 0.0f, 0.0f, __int_as_float(-1));
	if (i >= 0) {
		const float* tn = tris + (size_t)i * 12 + 9;
		f3 nn = mk3(tn[0], tn[1], tn[2]);
		const f3 dir = mk3(rays[(size_t)p * 6 + 3], rays[(size_t)p * 6 + 4], rays[(size_t)p * 6 + 5]);
		if (dot3(nn, dir) > 0.0f) nn = scale3(nn, -1.0f);            // as the path kernels orient it (sp_kernels.h)
		if constexpr (IsNorm<Norm...>::value) {
			const f3 o = mk3(rays[(size_t)p * 6], rays[(size_t)p * 6 + 1], rays[(size_t)p * 6 + 2]);
			const f3 ng = nn;
			(void)shade_normal(tris + (size_t)i * 12, norm_table(norm...) + (size_t)i * 9, o, dir, ng, nn);
			if constexpr (IsNmap<Norm...>::value) {                    // normal mapping: NormArgs, NmapArgs (k_gbuffer_nmap)
				const NmapArgs& x = pack_get<NmapArgs>(norm...);
				const float4 r = nmap_normal(tris + (size_t)i * 12, x.uv + (size_t)i * 6, x.nmap, x.nw, x.nh, o, dir, ng, nn);
				nn = mk3(r.x, r.y, r.z);
			}
		}
		const float* m = mats + (size_t)i * 6;
		g0 = make_float4(nn.x, nn.y, nn.z, dist[p]);
		g1 = make_float4(m[0], m[1], m[2], __int_as_float(cls[i]));
	}
	out[(size_t)p * 2] = g0;
	out[(size_t)p * 2 + 1] = g1;
}
__global__ void __launch_bounds__(256) k_gbuffer(const float* __restrict__ rays, const int* __restrict__ idx, const float* __restrict__ dist,
                                                 const float* __restrict__ tris, const float* __restrict__ mats, const int* __restrict__ cls,
                                                 uint32_t n, float4* __restrict__ out) {
	gbuffer_entry(rays, idx, dist, tris, mats, cls, n, out);
}
__global__ void __launch_bounds__(256) k_gbuffer_smooth(const float* __restrict__ rays, const int* __restrict__ idx, const float* __restrict__ dist,
                                                        const float* __restrict__ tris, const float* __restrict__ mats, const int* __restrict__ cls,
                                                        uint32_t n, float4* __restrict__ out, const NormArgs norm) {
	gbuffer_entry(rays, idx, dist, tris, mats, cls, n, out, norm);
}
// normal mapping: the perturbed shading normal of the primary ray; norm's table is the scene's vertex normals or zeros
__global__ void __launch_bounds__(256) k_gbuffer_nmap(const float* __restrict__ rays, const int* __restrict__ idx, const float* __restrict__ dist,
                                                      const float* __restrict__ tris, const float* __restrict__ mats, const int* __restrict__ cls,
                                                      uint32_t n, float4* __restrict__ out, const NormArgs norm, const NmapArgs nmap) {
	gbuffer_entry(rays, idx, dist, tris, mats, cls, n, out, norm, nmap);
}

SP_DEV void dn_emit(uint32_t p, float r, float g, float b, uint32_t* __restrict__ rgba, float* __restrict__ rgb) {
	if (rgba) rgba[p] = clamped_rgba(mk3(r, g, b));
	if (rgb) { rgb[(size_t)p * 3 + 0] = r; rgb[(size_t)p * 3 + 1] = g; rgb[(size_t)p * 3 + 2] = b; }
}

// caller's mean (3 f32) and variance (f32 or none: 0) -> float4; with K = 0 the outputs directly
__global__ void __launch_bounds__(256) k_dn_pack(const float* __restrict__ mean, const float* __restrict__ var, uint32_t n,
                                                 float4* __restrict__ out4, uint32_t* __restrict__ rgba, float* __restrict__ rgb) {
	const uint32_t p = blockIdx.x * 256u + threadIdx.x;
	if (p >= n) return;
	const float r = mean[(size_t)p * 3], g = mean[(size_t)p * 3 + 1], b = mean[(size_t)p * 3 + 2];
	if (out4) out4[p] = make_float4(r, g, b, var ? var[p] : 0.0f);
	dn_emit(p, r, g, b, rgba, rgb);
}

// a float4 image's outputs as they stand (K = 0 on a gathered frame)
__global__ void __launch_bounds__(256) k_dn_emit4(const float4* __restrict__ in4, uint32_t n, uint32_t* __restrict__ rgba, float* __restrict__ rgb) {
	const uint32_t p = blockIdx.x * 256u + threadIdx.x;
	if (p >= n) return;
	const float4 v = in4[p];
	dn_emit(p, v.x, v.y, v.z, rgba, rgb);
}

// an accumulation's state -> float4 {mean, var}.  Mean: the resolve of the path kernels (sum * float(1.0 / count)).  Variance
// of the mean (s12 != nullptr, adaptive): with the rule's own m and v, (float)max(0, v / n) in double; +inf when n < 2.
__global__ void __launch_bounds__(256) k_dn_prep(const float* __restrict__ sum, const uint32_t* __restrict__ counts, uint32_t total,
                                                 const double* __restrict__ s12, uint32_t n, float4* __restrict__ out4,
                                                 uint32_t* __restrict__ rgba, float* __restrict__ rgb) {
	const uint32_t p = blockIdx.x * 256u + threadIdx.x;
	if (p >= n) return;
	const uint32_t c = counts ? counts[p] : total;
	const float inv_n = (float)(1.0 / (double)(c ? c : 1u));
	const f3 av = scale3(mk3(sum[(size_t)p * 3 + 0], sum[(size_t)p * 3 + 1], sum[(size_t)p * 3 + 2]), inv_n);
	float var = 0.0f;
	if (s12) {
		if (c < 2u) var = __int_as_float(0x7f800000);
		else {
			const double nn = (double)c, s1 = s12[(size_t)p * 2], s2 = s12[(size_t)p * 2 + 1];
			const double m = s1 / nn;
			const double v = (s2 - s1 * m) / (nn - 1.0);
			const double q = v / nn;
			var = (float)(q > 0.0 ? q : 0.0);
		}
	}
	out4[p] = make_float4(av.x, av.y, av.z, var);
	dn_emit(p, av.x, av.y, av.z, rgba, rgb);
}

struct AtrousArgs {
	const float4* in;
	float4* out;
	const float4* gbuf;
	uint32_t w, h;
	int s;                  // step 2^i
	float zs;               // sigma_depth * s
	float sl2;              // sigma_lum * sigma_lum
	uint32_t normal_log2;
	uint32_t use_var;       // 0: no variance, wl = 1
	uint32_t* rgba;         // last iteration: the outputs (else nullptr)
	float* rgb;
};

// B3-spline taps {1/16, 1/4, 3/8, 1/4, 1/16} (selects, not an indexed array: no scratch)
SP_DEV float atrous_h(int d) { return d == 0 ? 0.375f : ((d == 1 || d == -1) ? 0.25f : 0.0625f); }

constexpr int kTapOutside = -0x7fffffff - 1;   // class of a staged tap outside the image: equal to no hit's class

// the stated weight of a non-centre tap q of hit pixel p (mat_q == mat_p already checked); lp, zden, lden, lum: p's terms
SP_DEV float atrous_weight(int dx, int dy, float4 gp0, float4 gq0, float4 cq, float lp, float zden, float lden, bool lum, uint32_t normal_log2) {
	const float d = (gp0.x * gq0.x + gp0.y * gq0.y) + gp0.z * gq0.z;
	float wn = d > 0.0f ? d : 0.0f;
	for (uint32_t k = 0; k < normal_log2; ++k) wn = wn * wn;
	const float dd = fabsf(gp0.w - gq0.w);
	float wz;
	if (zden == 0.0f) wz = dd == 0.0f ? 1.0f : 0.0f;
	else { const float t = 1.0f - dd / zden; wz = t > 0.0f ? t : 0.0f; }
	float wl = 1.0f;
	if (lum) {
		const float dl = lp - ((cq.x + cq.y) + cq.z);
		if (lden == 0.0f) wl = dl == 0.0f ? 1.0f : 0.0f;
		else { const float t = 1.0f - (dl * dl) / lden; wl = t > 0.0f ? t : 0.0f; }
	}
	return (((atrous_h(dx) * atrous_h(dy)) * wn) * wz) * wl;
}

// the sums of one hit pixel over its 25 taps, in tap order; TAP(dx, dy, cq, gq0, mq) fetches tap (dx, dy) and returns false when
// it lies outside the image
template <class Tap>
SP_DEV float4 atrous_pixel(const AtrousArgs& A, float4 cp, float4 gp0, int matp, const Tap& tap) {
	const float lp = (cp.x + cp.y) + cp.z;
	const float zden = A.zs * gp0.w;                                   // (sigma_z * s) * d_p
	const float lden = A.sl2 * cp.w;                                   // sigma_l^2 * var_p
	const bool lum = A.use_var && !(cp.w == __int_as_float(0x7f800000));
	float W = 0.0f, Cr = 0.0f, Cg = 0.0f, Cb = 0.0f, V = 0.0f;
	for (int dy = -2; dy <= 2; ++dy) {
		for (int dx = -2; dx <= 2; ++dx) {
			float w;
			float4 cq;
			if (dx == 0 && dy == 0) {
				w = 0.140625f;                                         // 9/64: the centre tap's edge weights are 1
				cq = cp;
			} else {
				float4 gq0;
				int mq;
				if (!tap(dx, dy, cq, gq0, mq)) continue;               // outside the image
				if (mq != matp) continue;                              // wm = 0
				w = atrous_weight(dx, dy, gp0, gq0, cq, lp, zden, lden, lum, A.normal_log2);
			}
			const float ww = w * w;
			if (!(ww > 0.0f)) continue;                                // a tap counts only when w * w > 0
			W = W + w;
			Cr = Cr + w * cq.x;
			Cg = Cg + w * cq.y;
			Cb = Cb + w * cq.z;
			V = V + ww * cq.w;
		}
	}
	return make_float4(Cr / W, Cg / W, Cb / W, V / (W * W));
}

// one a-trous iteration, taps read through the caches: 16 x 16 pixels per workgroup
__global__ void __launch_bounds__(256) k_atrous(const AtrousArgs A) {
	const int x = (int)(blockIdx.x * 16u + (threadIdx.x & 15u)), y = (int)(blockIdx.y * 16u + (threadIdx.x >> 4));
	if (x >= (int)A.w || y >= (int)A.h) return;
	const size_t p = (size_t)y * A.w + (size_t)x;
	const float4 cp = A.in[p];
	const float4 gp0 = A.gbuf[p * 2];
	const int matp = __float_as_int(A.gbuf[p * 2 + 1].w);
	float4 res = cp;                                                   // miss pixels pass through
	if (matp >= 0)
		res = atrous_pixel(A, cp, gp0, matp, [&](int dx, int dy, float4& cq, float4& gq0, int& mq) -> bool {
			const int yy = y + A.s * dy, xx = x + A.s * dx;
			if (yy < 0 || yy >= (int)A.h || xx < 0 || xx >= (int)A.w) return false;
			const size_t q = (size_t)yy * A.w + (size_t)xx;
			mq = __float_as_int(A.gbuf[q * 2 + 1].w);
			if (mq != matp) return true;                               // not read further: the caller skips it
			gq0 = A.gbuf[q * 2];
			cq = A.in[q];
			return true;
		});
	A.out[p] = res;
	if (A.rgba) dn_emit((uint32_t)p, res.x, res.y, res.z, A.rgba, A.rgb);
}

// the same iteration with the taps staged in LDS: a workgroup takes a 16 x 16 block of one stride-s sub-lattice (pixels
// (rx + s u, ry + s v)), whose taps form the dense 20 x 20 block around it on the same sub-lattice; each tap's colour, normal,
// distance and class are loaded once (36 B x 400 = 14.4 KB).  Grid: x = (tile column) * s + rx, y = (tile row) * s + ry.
__global__ void __launch_bounds__(256) k_atrous_lds(const AtrousArgs A) {
	__shared__ float4 s_c[400], s_g[400];
	__shared__ int s_m[400];
	const int s = A.s;
	const int rx = (int)(blockIdx.x % (uint32_t)s), ry = (int)(blockIdx.y % (uint32_t)s);
	const int u0 = (int)(blockIdx.x / (uint32_t)s) * 16, v0 = (int)(blockIdx.y / (uint32_t)s) * 16;
	for (int i = (int)threadIdx.x; i < 400; i += 256) {
		const int x = rx + s * (u0 + i % 20 - 2), y = ry + s * (v0 + i / 20 - 2);
		if (x >= 0 && x < (int)A.w && y >= 0 && y < (int)A.h) {
			const size_t q = (size_t)y * A.w + (size_t)x;
			s_c[i] = A.in[q];
			s_g[i] = A.gbuf[q * 2];
			s_m[i] = __float_as_int(A.gbuf[q * 2 + 1].w);
		} else s_m[i] = kTapOutside;                                       // outside the image
	}
	__syncthreads();
	const int tu = (int)(threadIdx.x & 15u), tv = (int)(threadIdx.x >> 4);
	const int x = rx + s * (u0 + tu), y = ry + s * (v0 + tv);
	if (x >= (int)A.w || y >= (int)A.h) return;
	const size_t p = (size_t)y * A.w + (size_t)x;
	const int c = (tv + 2) * 20 + tu + 2;
	const float4 cp = s_c[c];
	const int matp = s_m[c];
	float4 res = cp;
	if (matp >= 0)
		res = atrous_pixel(A, cp, s_g[c], matp, [&](int dx, int dy, float4& cq, float4& gq0, int& mq) -> bool {
			const int i = c + dy * 20 + dx;
			mq = s_m[i];
			if (mq == kTapOutside) return false;
			cq = s_c[i];
			gq0 = s_g[i];
			return true;
		});
	A.out[p] = res;
	if (A.rgba) dn_emit((uint32_t)p, res.x, res.y, res.z, A.rgba, A.rgb);
}

} // namespace sp
