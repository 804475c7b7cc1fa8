// Environment lighting (include/spath_hip.h "environment lighting"): an octahedral radiance map beside the
// scene, n x n RGB texels over (a, b) in [-1, 1]^2 with +y at the centre, and the tables that importance-sample it.
//
// Here: the kernels that build the importance tables behind both setters, and the test-only kernels of sphip_selftest_device what 9
// and 10.  The device functions a path calls (env_lookup, env_sample, env_miss, env_light) are in sp_integrator.h with the rest of
// the integrator's arithmetic.
#pragma once

#include "sp_integrator.h"

namespace sp {

// ---- the importance tables, in double, sequential where the order of the additions is the contract (numpy's cumsum)

// wt[t] = (((double)R + G) + B) / |g_c|^3, g_c the octahedron point of the texel's centre: the texel's radiance times its solid angle
// per unit (a, b) area
__global__ void __launch_bounds__(256) k_env_wt(const float* __restrict__ texels, uint32_t n, double* __restrict__ wt) {
	const uint32_t t = blockIdx.x * 256u + threadIdx.x;
	if (t >= n * n) return;
	const uint32_t i = t % n, j = t / n;
	const double a = -1.0 + (double)(2u * i + 1u) / (double)n, b = -1.0 + (double)(2u * j + 1u) / (double)n;
	const double y = (1.0 - __builtin_fabs(a)) - __builtin_fabs(b);
	double x = a, z = b;
	if (!(y >= 0.0)) {
		x = (1.0 - __builtin_fabs(b)) * (a < 0.0 ? -1.0 : 1.0);
		z = (1.0 - __builtin_fabs(a)) * (b < 0.0 ? -1.0 : 1.0);
	}
	const double l2 = (x * x + y * y) + z * z;
	const float* q = texels + (size_t)t * 3;
	wt[t] = (((double)q[0] + (double)q[1]) + (double)q[2]) / (__builtin_sqrt(l2) * l2);
}

// rc[j][i] = wt[j][0] + ... + wt[j][i], added in that order: one thread per row.  Neighbouring lanes read wt n doubles apart, which is
// uncoalesced; it is what the sequential order costs, off the hot path (about a millisecond at n = 2048): not a pattern to copy
__global__ void __launch_bounds__(256) k_env_rows(const double* __restrict__ wt, uint32_t n, double* __restrict__ rc) {
	const uint32_t j = blockIdx.x * 256u + threadIdx.x;
	if (j >= n) return;
	double s = 0.0;
	for (uint32_t i = 0; i < n; ++i) {
		s = s + wt[(size_t)j * n + i];
		rc[(size_t)j * n + i] = s;
	}
}

// marg[j] = rc[0][n - 1] + ... + rc[j][n - 1], added in that order: one thread
__global__ void k_env_marg(const double* __restrict__ rc, uint32_t n, double* __restrict__ marg) {
	if (blockIdx.x != 0 || threadIdx.x != 0) return;
	double s = 0.0;
	for (uint32_t j = 0; j < n; ++j) {
		s = s + rc[(size_t)j * n + (n - 1u)];
		marg[j] = s;
	}
}

// tpdf[t] = (float)((sel * (wt[t] / T)) * area): sel = w_env / W, the probability that the light table picks the environment, area =
// n n / 4, texels per unit (a, b) area.  sel = 0 (no entry: a black map): zeros
__global__ void __launch_bounds__(256) k_env_tpdf(const double* __restrict__ wt, uint32_t n, double sel, double T, float* __restrict__ tpdf) {
	const uint32_t t = blockIdx.x * 256u + threadIdx.x;
	if (t >= n * n) return;
	const double area = (double)n * (double)n / 4.0;
	tpdf[t] = sel > 0.0 ? (float)((sel * (wt[t] / T)) * area) : 0.0f;
}

// ---- test-only (sphip_selftest_device).  what 9: env_lookup.  d.xyz -> i, j, r3, valid
__global__ void __launch_bounds__(256) k_selftest_env_lookup(const float* __restrict__ in, uint32_t m, uint32_t n, float* __restrict__ out) {
	const uint32_t k = blockIdx.x * 256u + threadIdx.x;
	if (k >= m) return;
	const float* q = in + 3 * (size_t)k;
	uint32_t i, j;
	float r3;
	const bool ok = env_lookup(mk3(q[0], q[1], q[2]), n, i, j, r3);
	float* w = out + 4 * (size_t)k;
	w[0] = (float)i; w[1] = (float)j; w[2] = r3; w[3] = ok ? 1.0f : 0.0f;
}

// what 10: env_sample.  r8 r9 r3 r4 -> i, j, wd.xyz, r3
__global__ void __launch_bounds__(256) k_selftest_env_sample(const double* __restrict__ in, uint32_t m, const EnvMap e, float* __restrict__ out) {
	const uint32_t k = blockIdx.x * 256u + threadIdx.x;
	if (k >= m) return;
	const double* q = in + 4 * (size_t)k;
	uint32_t i, j;
	f3 wd;
	float r3;
	env_sample(e, q[0], q[1], q[2], q[3], i, j, wd, r3);
	float* w = out + 6 * (size_t)k;
	w[0] = (float)i; w[1] = (float)j; w[2] = wd.x; w[3] = wd.y; w[4] = wd.z; w[5] = r3;
}

} // namespace sp
