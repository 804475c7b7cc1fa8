// Temporal reprojection (include/spath_hip.h: sphip_reproject_device, sphip_temporal_resolve_device, sphip_accum_reproject;
// DESIGN.md section 5.19): the previous view's accumulated radiance resampled at the new view's primary hits, and its blend with
// the new view's samples.  A post-process like the denoiser: nothing here is reached by the scan or path kernels.
//
// Every operation below is an f32 + - * / (IEEE division), a comparison, a select or a float-to-int floor, in the order the header
// states, so that a numpy model replays the output bit for bit (the build has -ffp-contract=off: nothing is fused).
//
// Layouts: ray = 6 f32 pos.xyz dir.xyz; G-buffer entry = two float4 {nx, ny, nz, dist}, {ar, ag, ab, mat as i32 bits} (sp_denoise.h);
// mean = 3 f32 per pixel; history count = 1 f32 per pixel.
//
// One pass, taps read through the caches.  The four taps of a lane lie where the reprojection puts them, so unlike the a-trous
// filter's there is no tile that a workgroup could stage before it knows them; for the camera moves this is made for, the taps of
// neighbouring lanes are neighbouring entries, and each 32 B G-buffer entry or 24 B ray is a whole number of 16 B / 8 B loads.
#pragma once

#include "sp_denoise.h"

namespace sp {

struct ReprojArgs {
	const float* rays_cur;
	const float4* gbuf_cur;
	const float* rays_prev;
	const float4* gbuf_prev;
	const float* mean_prev;
	const float* hist_prev;
	float* out_mean;
	float* out_hist;
	uint32_t w, h, n;
	// the previous camera: position, rotation, focal, and the viewport constants of view_args (xo = x_max - h_x_step, yo likewise)
	float px, py, pz, cos_y, sin_y, cos_x, sin_x, focal;
	float xo, x_step, yo, y_step;
	float max_history, normal_min, plane_tol;
};

// o + d * t per component: one multiply, one add
SP_DEV f3 rp_point(const float* __restrict__ ray, float t) {
	return mk3(ray[0] + ray[3] * t, ray[1] + ray[4] * t, ray[2] + ray[5] * t);
}

SP_DEV void rp_emit(const ReprojArgs& A, uint32_t p, float r, float g, float b, float hist) {
	A.out_mean[(size_t)p * 3 + 0] = r; A.out_mean[(size_t)p * 3 + 1] = g; A.out_mean[(size_t)p * 3 + 2] = b;
	A.out_hist[p] = hist;
}

__global__ void __launch_bounds__(256) k_reproject(const ReprojArgs A) {
	const uint32_t p = blockIdx.x * 256u + threadIdx.x;
	if (p >= A.n) return;
	const float4 g0 = A.gbuf_cur[(size_t)p * 2], g1 = A.gbuf_cur[(size_t)p * 2 + 1];
	const int matp = __float_as_int(g1.w);
	if (matp < 0) { rp_emit(A, p, 0.0f, 0.0f, 0.0f, 0.0f); return; }                 // 1. miss
	const f3 np = mk3(g0.x, g0.y, g0.z);
	const float distp = g0.w;
	const f3 P = rp_point(A.rays_cur + (size_t)p * 6, distp);                        // 2.
	const f3 v = mk3(P.x - A.px, P.y - A.py, P.z - A.pz);                            // 3. rY^-1, then rX^-1
	const f3 a = mk3(v.x * A.cos_y + v.z * -A.sin_y, v.y, v.x * A.sin_y + v.z * A.cos_y);
	const f3 c = mk3(a.x, a.y * A.cos_x + a.z * A.sin_x, a.y * -A.sin_x + a.z * A.cos_x);
	if (!(c.z > 0.0f)) { rp_emit(A, p, 0.0f, 0.0f, 0.0f, 0.0f); return; }             // behind the previous view plane
	const float qz = c.z + A.focal;
	const float sx = (c.x * A.focal) / qz, sy = (c.y * A.focal) / qz;
	const float fx = (A.xo - sx) / A.x_step, fy = (A.yo - sy) / A.y_step;            // 4.
	const float inf = __int_as_float(0x7f800000);
	if (!(fabsf(fx) < inf) || !(fabsf(fy) < inf)) { rp_emit(A, p, 0.0f, 0.0f, 0.0f, 0.0f); return; }
	const float x0f = floorf(fx), y0f = floorf(fy);
	const float tx = fx - x0f, ty = fy - y0f;
	// a footprint wholly off the frame has no tap; what is left converts to int exactly (w, h < 2^30)
	if (!(x0f >= -1.0f && x0f < (float)A.w && y0f >= -1.0f && y0f < (float)A.h)) { rp_emit(A, p, 0.0f, 0.0f, 0.0f, 0.0f); return; }
	const int x0 = (int)x0f, y0 = (int)y0f;
	const float ux = 1.0f - tx, uy = 1.0f - ty;
	const float ptd = A.plane_tol * distp;
	float W = 0.0f, Cr = 0.0f, Cg = 0.0f, Cb = 0.0f, Hs = 0.0f;
	for (int b = 0; b < 2; ++b) {                                                      // 5.
		for (int aa = 0; aa < 2; ++aa) {
			const int xx = x0 + aa, yy = y0 + b;
			if (xx < 0 || xx >= (int)A.w || yy < 0 || yy >= (int)A.h) continue;        // nothing of a tap is read before this
			const float wb = (aa ? tx : ux) * (b ? ty : uy);
			if (!(wb > 0.0f)) continue;
			const size_t q = (size_t)yy * A.w + (size_t)xx;
			const float hq = A.hist_prev[q];
			if (!(hq > 0.0f)) continue;
			const float4 q1 = A.gbuf_prev[q * 2 + 1];
			if (__float_as_int(q1.w) != matp) continue;
			const float4 q0 = A.gbuf_prev[q * 2];
			const float dn = (np.x * q0.x + np.y * q0.y) + np.z * q0.z;
			if (!(dn >= A.normal_min)) continue;
			const f3 Pq = rp_point(A.rays_prev + q * 6, q0.w);
			const f3 e = mk3(Pq.x - P.x, Pq.y - P.y, Pq.z - P.z);
			const float pd = (e.x * np.x + e.y * np.y) + e.z * np.z;
			if (!(fabsf(pd) <= ptd)) continue;
			W = W + wb;
			Cr = Cr + wb * A.mean_prev[q * 3 + 0];
			Cg = Cg + wb * A.mean_prev[q * 3 + 1];
			Cb = Cb + wb * A.mean_prev[q * 3 + 2];
			Hs = Hs + wb * hq;
		}
	}
	if (!(W > 0.0f)) { rp_emit(A, p, 0.0f, 0.0f, 0.0f, 0.0f); return; }               // 6.
	float hist = Hs / W;
	hist = hist > A.max_history ? A.max_history : hist;
	rp_emit(A, p, Cr / W, Cg / W, Cb / W, hist);
}

// the blend of a history (hm, h) with the running sum s of n new samples, per channel; h == 0: the resolve of the path kernels
SP_DEV f3 rp_blend(f3 s, float inv_n, float fn, const float* __restrict__ hmean, const float* __restrict__ hist, uint32_t p) {
	const float h = hist ? hist[p] : 0.0f;
	if (h == 0.0f) return scale3(s, inv_n);
	const float den = h + fn;
	return mk3((h * hmean[(size_t)p * 3 + 0] + s.x) / den, (h * hmean[(size_t)p * 3 + 1] + s.y) / den, (h * hmean[(size_t)p * 3 + 2] + s.z) / den);
}

// sum of n_samples samples + history -> RGBA8 and mean (each may be nullptr).  inv_n = float(1.0 / n_samples) and fn = (float)n_samples,
// formed by the host; hist == nullptr: no pixel has a history
__global__ void __launch_bounds__(256) k_temporal_resolve(const float* __restrict__ sum, float inv_n, float fn, const float* __restrict__ hmean,
                                                          const float* __restrict__ hist, uint32_t n, uint32_t* __restrict__ rgba, float* __restrict__ mean) {
	const uint32_t p = blockIdx.x * 256u + threadIdx.x;
	if (p >= n) return;
	const f3 av = rp_blend(mk3(sum[(size_t)p * 3 + 0], sum[(size_t)p * 3 + 1], sum[(size_t)p * 3 + 2]), inv_n, fn, hmean, hist, p);
	dn_emit(p, av.x, av.y, av.z, rgba, mean);
}

// a finished accumulation (sum of `total` samples, its own history or none) -> the (mean, hist) pair the next reprojection reads:
// mean = the blend above, hist = its history + (float)total.  The cap is k_reproject's.
__global__ void __launch_bounds__(256) k_history(const float* __restrict__ sum, float inv_n, float fn, const float* __restrict__ hmean,
                                                 const float* __restrict__ hist, uint32_t n, float* __restrict__ out_mean, float* __restrict__ out_hist) {
	const uint32_t p = blockIdx.x * 256u + threadIdx.x;
	if (p >= n) return;
	const f3 av = rp_blend(mk3(sum[(size_t)p * 3 + 0], sum[(size_t)p * 3 + 1], sum[(size_t)p * 3 + 2]), inv_n, fn, hmean, hist, p);
	out_mean[(size_t)p * 3 + 0] = av.x; out_mean[(size_t)p * 3 + 1] = av.y; out_mean[(size_t)p * 3 + 2] = av.z;
	out_hist[p] = (hist ? hist[p] : 0.0f) + fn;
}

} // namespace sp
